// mc_bp_dbg.inl — S1 back-projection, bp_launch_denoise: the diagnostics build's invariant checks
// (included by mc_bp_denoise_lds.inl after the helpers they recompute from; compiled to nothing but
// their counters in every other build).
namespace mc {

// ---------------------------------------------------------------------------------------------
// Diagnostics build only (-DMC_DBG_CHECK=1: scripts/build_variant.sh dbg): invariant checks inside the
// LDS denoise classes, each against a direct recomputation from the cell-sorted points.  Kinds:
//   0  a point's eps-neighbour count != the points within eps in its 27 cells
//   1  a list the consumers read (count <= nbcap) whose entries (position | radius class) differ
//      from those points as a multiset (sum and xor of a 64-bit mix of each entry)
//   2  two core points within eps in different union-find components
//   3  a kept point's mean k-NN distance != the brute-force mean over every kept point (bits; checked in
//      k_bp_denoise_tail, after the ring-search kernel)
// Each failure is counted in g_bp_dbg[kind] (read by mc_debug_counters) and the first 16 printed.
// ---------------------------------------------------------------------------------------------
#ifndef MC_DBG_CHECK
#define MC_DBG_CHECK 0
#endif
#ifndef MC_DBG_NOINLINE
#define MC_DBG_NOINLINE 1  // 0: the checks inlined (which of the two builds clean depends on the source:
                           //    scripts/build_variant.sh rejects one with misplaced spills)
#endif
#ifndef MC_DBG_PRINT
#define MC_DBG_PRINT 1     // 0: failures counted only (no device printf)
#endif
#if MC_DBG_NOINLINE
#define MC_DBG_FN __device__ __noinline__
#else
#define MC_DBG_FN __device__ __forceinline__
#endif
__device__ unsigned long long g_bp_dbg[8];
__device__ unsigned g_bp_dbg_printed;
// (diagnostics build) which step produced each kept point's k-NN mean, by batch pixel index base + rank:
// 1 list pass, 2 whole cloud (m < k), 3 whole cloud (queue region full), 4 ring-search kernel; the
// list pass also records the class size N and the list count
constexpr int kBpDbgPath = MC_DBG_CHECK ? (1 << 24) : 1;
__device__ unsigned g_bp_dbg_path[kBpDbgPath];
__device__ __forceinline__ void bp_dbg_path(size_t i, unsigned code)
{
    if (MC_DBG_CHECK && i < static_cast<size_t>(kBpDbgPath)) g_bp_dbg_path[i] = code;
}
__device__ __forceinline__ bool bp_dbg_fail(int kind)
{
    atomicAdd(&g_bp_dbg[kind], 1ull);
    return MC_DBG_PRINT && atomicAdd(&g_bp_dbg_printed, 1u) < 16u;
}
__device__ __forceinline__ unsigned long long bp_dbg_mix(unsigned long long k)
{
    k *= 0x9E3779B97F4A7C15ull;
    k ^= k >> 29;
    k *= 0xBF58476D1CE4E5B9ull;
    return k ^ (k >> 32);
}
template <int N>
MC_DBG_FN void bp_dbg_lists(const BpLdsGrid &g, const int *sflag, const unsigned short *nbw, int n,
                                          const BpDev &pr, int slot)
{
    for (int q = threadIdx.x; q < n; q += blockDim.x) {
        const double4 a = g.pt[q];
        int x, y, z;
        unpack3(static_cast<unsigned long long>(__double_as_longlong(a.w)) & ~kKeptBit, x, y, z);
        int c = 0;
        unsigned long long sum = 0, xr = 0;
        lds_cells27(g, x, y, z, 0ull, a.x, a.y, a.z, [&](int q2, double d2) {
            if (d2 < pr.eps2) {
                const unsigned long long e = static_cast<unsigned>(q2) | (nb_class<N>(d2, pr) << kNbShift<N>);
                c++;
                sum += bp_dbg_mix(e);
                xr ^= bp_dbg_mix(e + 0x51ED2701ull);
            }
        });
        const int cnt = nb_cnt(sflag[q]);
        if (cnt != c) {
            if (bp_dbg_fail(0)) printf("[bp dbg] N=%d slot=%d n=%d q=%d: list count %d, cells %d\n", N, slot, n, q, cnt, c);
            continue;
        }
        if (cnt > pr.nbcap) continue;
        unsigned long long s2 = 0, x2 = 0;
        for (int k = 0; k < cnt; k++) {
            const unsigned long long e = nbw[(static_cast<size_t>(k >> 3) * N + q) * 8 + (k & 7)];
            s2 += bp_dbg_mix(e);
            x2 ^= bp_dbg_mix(e + 0x51ED2701ull);
        }
        if (s2 != sum || x2 != xr)
            if (bp_dbg_fail(1)) printf("[bp dbg] N=%d slot=%d n=%d q=%d: list entries differ (count %d)\n", N, slot, n, q, cnt);
    }
    sync_global();
}
template <int N>
MC_DBG_FN void bp_dbg_union(const BpLdsGrid &g, const int *spar, int n, const BpDev &pr, int slot)
{
    for (int q = threadIdx.x; q < n; q += blockDim.x) {
        const int ra = spar[q];
        if (ra < 0) continue;
        const double4 a = g.pt[q];
        int x, y, z;
        unpack3(static_cast<unsigned long long>(__double_as_longlong(a.w)) & ~kKeptBit, x, y, z);
        lds_cells27(g, x, y, z, 0ull, a.x, a.y, a.z, [&](int q2, double d2) {
            const int rb = spar[q2];
            if (d2 < pr.eps2 && rb >= 0 && rb != ra)
                if (bp_dbg_fail(2)) printf("[bp dbg] N=%d slot=%d n=%d: core %d (root %d) and %d (root %d) apart\n", N, slot, n,
                                           q, ra, q2, rb);
        });
    }
    sync_global();
}
// (in k_bp_denoise_tail, a wave per slot) kept point of rank r: original index sx[r], mean av[r]
MC_DBG_FN void bp_dbg_knn_tail(const double *P, const int *sx, const double *av, int m, int kk, int slot,
                                             int base)
{
    for (int r = lane_id(); r < m; r += 64) {
        const double *a = P + 3 * sx[r];
        double best[kBpKnnMax];
        for (int k = 0; k < kBpKnnMax; k++) best[k] = DBL_MAX;
        for (int j = 0; j < m; j++) {
            const double *p = P + 3 * sx[j];
            const double ex = a[0] - p[0], ey = a[1] - p[1], ez = a[2] - p[2];
            sorted_insert(best, ((ex * ex) + (ey * ey)) + (ez * ez));
        }
        double sum = 0.0;
        for (int k = 0; k < kk; k++) sum = sum + sqrt(best[k]);
        const double want = sum / static_cast<double>(kk), got = av[r];
        if (__double_as_longlong(want) != __double_as_longlong(got))
            if (bp_dbg_fail(3)) {
                const size_t gi = static_cast<size_t>(base) + r;
                const unsigned pc = gi < static_cast<size_t>(kBpDbgPath) ? g_bp_dbg_path[gi] : 0u;
                printf("[bp dbg] slot=%d m=%d r=%d: k-NN mean %.17g, brute force %.17g (path %u, class N %u, list count %u)\n",
                       slot, m, r, got, want, pc & 0xFu, (pc >> 4) & 0xFFFFu, pc >> 20);
            }
    }
}

}  // namespace mc
