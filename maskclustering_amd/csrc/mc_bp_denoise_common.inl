// mc_bp_denoise_common.inl — S1 back-projection, bp_launch_denoise: what the LDS classes
// (mc_bp_denoise_lds.inl) and the global-memory kernels (mc_bp_denoise.inl) share: the hashed cell
// grid's walks, union-find, the k-NN mean and the ordered sums.
namespace mc {

// ---------------------------------------------------------------------------------------------
// (a4) denoise (geometry.py:9-24), workgroup per slot
// ---------------------------------------------------------------------------------------------
// Points are bucketed into a hashed grid of cells ce = 1.01 eps (2 buckets per point, counting
// sort); a point is visited only from its own cell (the cell key is compared), so every
// neighbourhood scan sees each point once.
//   DBSCAN (Open3D ClusterDBSCAN): core = >= min_points neighbours with d2 < eps^2 (self
//   included); clusters = connected core points, numbered in order of their smallest point (the
//   order Open3D seeds them); a non-core point with a core neighbour joins the lowest-numbered
//   adjacent cluster (the first cluster to reach it), else it is noise.
//   Class filter: drop every label class (noise included) with count < 0.2 n.
//   remove_statistical_outlier(20, 2): mean distance to the k = min(20, m) nearest points of the
//   kept set (self included, sqrt'ed and summed in ascending order), cloud mean and Bessel std
//   as sequential sums in index order, keep 0 < d < mean + 2 std.
struct BpCells {
    const unsigned long long *pc;
    const int *bs, *bl;
    unsigned nb;
    int cmax[3];
};

// calls fn(j) for every point j in cell (x, y, z) (no-op outside the grid)
template <typename Fn>
__device__ __forceinline__ void bp_cell_points(const BpCells &g, int x, int y, int z, Fn &&fn)
{
    if (x < 0 || y < 0 || z < 0 || x > g.cmax[0] || y > g.cmax[1] || z > g.cmax[2]) return;
    const unsigned long long key = pack3(x, y, z);
    const unsigned b = mod_mul(bp_hash3(x, y, z), g.nb);
    for (int k = g.bs[b]; k < g.bs[b + 1]; k++) {
        const int j = g.bl[k];
        if (g.pc[j] == key) fn(j);
    }
}

// every point j in the (2R+1)^3 block of cells whose Chebyshev ring index is exactly R
template <typename Fn>
__device__ __forceinline__ void bp_shell(const BpCells &g, int cx, int cy, int cz, int R, Fn &&fn)
{
    for (int dz = -R; dz <= R; dz++)
        for (int dy = -R; dy <= R; dy++) {
            const bool edge = dz == -R || dz == R || dy == -R || dy == R;
            for (int dx = -R; dx <= R; dx += (edge || R == 0) ? 1 : 2 * R) bp_cell_points(g, cx + dx, cy + dy, cz + dz, fn);
        }
}

// union-find over a workgroup's LDS parent array (root = smallest index)
// (uf_find_s / uf_unite_s restate uf_find / uf_unite of mc_s6_columns.inl at workgroup scope)
constexpr int kBpLdsUF = 8192;
// (relaxed workgroup-scope atomic loads / stores: other lanes update the array concurrently, and
// unlike volatile they keep the LDS address space, i.e. ds_read / ds_write instead of flat ops)
__device__ __forceinline__ int ld_wg(int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_wg(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int uf_find_s(int *par, int x)
{
    while (true) {
        const int p = ld_wg(par + x);
        if (p == x) return x;
        const int gp = ld_wg(par + p);
        if (gp == p) return p;
        st_wg(par + x, gp);
        x = gp;
    }
}
__device__ __forceinline__ void uf_unite_s(int *par, int a, int b)
{
    while (true) {
        a = uf_find_s(par, a);
        b = uf_find_s(par, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        if (atomicCAS(par + b, b, a) == b) return;
    }
}

// Mean of sqrt of the kk smallest of d2(j) over j < m, by one wave: every lane keeps the
// kBpKnnMax smallest of its strided share, then kk rounds of a wave-wide minimum extract them in
// ascending order (the order Open3D sums them in).  d2fn(j) gives the j-th squared distance.
template <typename D2>
__device__ __forceinline__ double wave_knn_mean(int m, int kk, D2 &&d2fn)
{
    const int lane = lane_id();
    double loc[kBpKnnMax];
#pragma unroll
    for (int k = 0; k < kBpKnnMax; k++) loc[k] = DBL_MAX;
    for (int j = lane; j < m; j += 64) sorted_insert(loc, d2fn(j));
    double sum = 0.0;
    for (int k = 0; k < kk; k++) {
        double v = loc[0];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
        const int win = __ffsll(static_cast<long long>(__ballot(loc[0] == v))) - 1;
        sum = sum + sqrt(v);
        if (lane == win) {
#pragma unroll
            for (int q = 0; q < kBpKnnMax - 1; q++) loc[q] = loc[q + 1];
            loc[kBpKnnMax - 1] = DBL_MAX;
        }
    }
    return sum / static_cast<double>(kk);
}

// mean distance of every kept point to its k nearest kept points (self included): sqrt of the
// k smallest squared distances, summed in ascending order, / k (Open3D SearchKNN + accumulate)
template <int N>
__device__ __forceinline__ void bp_knn(const BpCells &g, const double *__restrict__ P, const int *__restrict__ flag,
                                       const int *__restrict__ si, int m, int kk, double ce, double *__restrict__ av,
                                       int t, int *fb, int fb_cap, int *nfb)
{
    constexpr int kRingMax = 2;
    if (t == 0) *nfb = 0;
    __syncthreads();
    for (int r = t; r < m; r += 256) {
        const int i = si[r];
        const unsigned long long key = g.pc[i];
        const int x = static_cast<int>(key >> 42), y = static_cast<int>((key >> 21) & 0x1FFFFF),
                  z = static_cast<int>(key & 0x1FFFFF);
        const double *pi = P + 3 * i;
        double best[N];
#pragma unroll
        for (int q = 0; q < N; q++) best[q] = DBL_MAX;
        int found = 0;
        bool done = false;
        // the ring search serves the full-k case only (kk == N: k-th smallest = best[N-1], a static
        // index; a dynamic one would mirror best[] into scratch on every insert); m < N goes to the
        // whole-wave path, which takes any kk
        for (int R = 0; R <= kRingMax && !done && kk == N; R++) {
            for (int dz = -R; dz <= R; dz++)
                for (int dy = -R; dy <= R; dy++) {
                    const bool edge = dz == -R || dz == R || dy == -R || dy == R;
                    const int step = (edge || R == 0) ? 1 : 2 * R;
                    for (int dx = -R; dx <= R; dx += step) {
                        const int cx = x + dx, cy = y + dy, cz = z + dz;
                        if (cx < 0 || cy < 0 || cz < 0 || cx > g.cmax[0] || cy > g.cmax[1] || cz > g.cmax[2]) continue;
                        const unsigned long long ck = pack3(cx, cy, cz);
                        const unsigned b = mod_mul(bp_hash3(cx, cy, cz), g.nb);
                        const int kb = g.bs[b], ke = g.bs[b + 1];
                        for (int k = kb; k < ke; k++) {
                            const int j = g.bl[k];
                            if (g.pc[j] != ck || !(flag[j] & (1 << 30))) continue;
                            sorted_insert(best, bp_d2(pi, P + 3 * j));
                            found++;
                        }
                    }
                }
            const double reach = static_cast<double>(R) * ce;
            done = found >= kk && best[N - 1] < reach * reach * (1.0 - 1e-9);
        }
        if (!done) {  // sparse point: every kept point, by a whole wave below
            const int f = atomicAdd(nfb, 1);
            if (f < fb_cap) {
                fb[f] = r;
                continue;
            }
#pragma unroll
            for (int q = 0; q < N; q++) best[q] = DBL_MAX;
            for (int q = 0; q < m; q++) sorted_insert(best, bp_d2(pi, P + 3 * si[q]));
        }
        double sum = 0.0;
#pragma unroll
        for (int q = 0; q < N; q++)
            if (q < kk) sum = sum + sqrt(best[q]);
        av[r] = sum / static_cast<double>(kk);
    }
    __syncthreads();
    const int nf = min(*nfb, fb_cap);
    for (int f = static_cast<int>(threadIdx.x >> 6); f < nf; f += 4) {
        const int r = fb[f];
        const double *pi = P + 3 * si[r];
        const double mean = wave_knn_mean(m, kk, [&](int j) { return bp_d2(pi, P + 3 * si[j]); });
        if (lane_id() == 0) av[r] = mean;
    }
}


// acc + v(lane 0) + v(lane 1) + ... + v(lane 63), in lane order, skipping lanes with v <= 0 (a
// std::accumulate step over 64 values); the lane values are read as scalars
template <bool kSkipNonPos = true>
__device__ __forceinline__ double seq_add64_pos(double acc, double v)
{
    const long long bits = __double_as_longlong(v);
    const int lo = static_cast<int>(bits), hi = static_cast<int>(bits >> 32);
#pragma unroll
    for (int j = 0; j < 64; j++) {
        const unsigned long long b = (static_cast<unsigned long long>(static_cast<unsigned>(__builtin_amdgcn_readlane(hi, j))) << 32) |
                                     static_cast<unsigned>(__builtin_amdgcn_readlane(lo, j));
        const double a = __longlong_as_double(static_cast<long long>(b));
        if (kSkipNonPos) {
            if (a > 0) acc = acc + a;
        } else {
            acc = acc + a;
        }
    }
    return acc;
}

}  // namespace mc
