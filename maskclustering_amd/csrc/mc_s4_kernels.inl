// mc_s4_kernels.inl — S4 observer-count histogram over ALL M masks (construction.py:84-86) and its
// percentiles (:88-95); included by mc_kernels.inl.  Launched by launch_hist, graph_thresholds and
// mc_observer_thresholds (mc_graph_host.inl).
namespace mc {

// Persistent blocks walk 64×64 (i, j) tiles of the upper triangle; O = popcount(VF_i & VF_j);
// positive O values are histogrammed with weight 2 off the diagonal (O is symmetric), 1 on it.
// Each block keeps R lane-indexed replicas of the histogram in LDS (no same-address
// atomics inside a wave) and reduces them once at the end.
constexpr int kHistTile = 64, kHistKW = 8;

// Word range [lo, hi] of the nonzero VF words of every 64-row tile (lo > hi: no visible frame).
// Masks are in frame order and each is visible in a window of frames, so far-apart tiles share no
// word and their observer counts are all 0 -- which the histogram of positive counts never needs.
__global__ __launch_bounds__(256) void k_s4_ranges(const unsigned long long *__restrict__ vf, int M, int FW, int nblk,
                                                   int2 *__restrict__ rng)
{
    const int lane = lane_id();
    for (int b = (blockIdx.x * 256 + threadIdx.x) >> 6; b < nblk; b += gridDim.x * 4) {
        const long long g = static_cast<long long>(b) * kHistTile + lane;
        int lo = INT_MAX, hi = -1;
        if (g < M)
            for (int w = 0; w < FW; w++)
                if (vf[static_cast<size_t>(g) * FW + w]) {
                    lo = min(lo, w);
                    hi = w;
                }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lo = min(lo, __shfl_xor(lo, d, 64));
            hi = max(hi, __shfl_xor(hi, d, 64));
        }
        if (lane == 0) rng[b] = make_int2(lo, hi);
    }
}

// shard_rank / shard_world: row-block sharding over processes — this rank takes
// every shard_world-th tile; the partial histograms are summed by the host's all-reduce.
__global__ __launch_bounds__(256) void k_s4_hist(const unsigned long long *__restrict__ vf, int M, int FW, int F,
                                                 int nblk, long long ntiles, int R, int HS,
                                                 const int2 *__restrict__ rng, unsigned long long *__restrict__ hist_g,
                                                 int shard_rank, int shard_world)
{
    extern __shared__ unsigned char smem_raw[];
    unsigned long long *A = reinterpret_cast<unsigned long long *>(smem_raw);
    unsigned long long *B = A + kHistTile * kHistKW;
    unsigned *hist = reinterpret_cast<unsigned *>(B + kHistTile * kHistKW);  // R replicas of HS (odd) bins

    for (int v = threadIdx.x; v < R * HS; v += 256) hist[v] = 0u;
    unsigned *myh = hist + (lane_id() & (R - 1)) * HS;
    const int ti = threadIdx.x >> 2;          // row in tile
    const int tj0 = (threadIdx.x & 3) * 16;   // 16 columns

    auto row_start = [&](long long r) { return r * nblk - (r * (r - 1)) / 2; };
    for (long long tile = static_cast<long long>(blockIdx.x) * shard_world + shard_rank; tile < ntiles;
         tile += static_cast<long long>(gridDim.x) * shard_world) {
        // triangular decode: tile -> (bi, bj), bi <= bj
        const double nn = nblk;
        long long bi = static_cast<long long>(floor((2.0 * nn + 1.0 - sqrt((2.0 * nn + 1.0) * (2.0 * nn + 1.0) - 8.0 * static_cast<double>(tile))) / 2.0));
        if (bi < 0) bi = 0;
        while (bi > 0 && row_start(bi) > tile) bi--;
        while (bi + 1 < nblk && row_start(bi + 1) <= tile) bi++;
        const long long bj = bi + (tile - row_start(bi));

        const int2 ri = rng[bi], rj = rng[bj];
        const int wlo = max(ri.x, rj.x), whi = min(ri.y, rj.y);
        if (wlo > whi) continue;  // no common word: every count of the tile is 0 (uniform)
        int acc[16];
#pragma unroll
        for (int k = 0; k < 16; k++) acc[k] = 0;
        for (int w0 = wlo; w0 <= whi; w0 += kHistKW) {
            __syncthreads();
            for (int x = threadIdx.x; x < kHistTile * kHistKW; x += 256) {
                const int r = x / kHistKW, w = x % kHistKW;
                const long long gi = bi * kHistTile + r, gj = bj * kHistTile + r;
                A[x] = (gi < M && w0 + w <= whi) ? vf[static_cast<size_t>(gi) * FW + w0 + w] : 0ull;
                B[x] = (gj < M && w0 + w <= whi) ? vf[static_cast<size_t>(gj) * FW + w0 + w] : 0ull;
            }
            __syncthreads();
            const int kw = min(kHistKW, whi + 1 - w0);
            for (int w = 0; w < kw; w++) {
                const unsigned long long a = A[ti * kHistKW + w];
#pragma unroll
                for (int k = 0; k < 16; k++) acc[k] += __popcll(a & B[(tj0 + k) * kHistKW + w]);
            }
        }
        const long long gi = bi * kHistTile + ti;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const long long gj = bj * kHistTile + tj0 + k;
            if (gi < M && gj < M && acc[k] > 0 && (bi != bj || gi <= gj)) atomicAdd(&myh[acc[k]], gi == gj ? 1u : 2u);
        }
    }
    __syncthreads();
    for (int v = threadIdx.x; v <= F; v += 256) {
        unsigned long long s = 0;
        for (int r = 0; r < R; r++) s += hist[r * HS + v];
        if (s) atomicAdd(&hist_g[v], s);
    }
}

// numpy 2.x np.percentile(float32 array, p), "linear" (see oracle/mcgraph_oracle.c and
// SURVEY.md App. A.4): every float op rounded explicitly (no contraction).  The
// histogram's cumulative counts are built in LDS; order statistics by binary search.
__device__ float cum_order_stat(const unsigned long long *cum, int F, unsigned long long k)
{
    // smallest v in [1, F] with cum[v] > k   (cum[v] = #values <= v)
    int lo = 1, hi = F;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > k) hi = mid;
        else lo = mid + 1;
    }
    return static_cast<float>(lo);
}

// dynamic LDS: cum[F+1] (u64); static: part and pval (kS4ThrStaticLds, which the host's limit check adds)
constexpr size_t kS4ThrStaticLds = 256 * sizeof(unsigned long long) + 20 * sizeof(float);
__global__ __launch_bounds__(256) void k_s4_thresholds(const unsigned long long *__restrict__ hist, int F,
                                                       float *__restrict__ thr, int *__restrict__ is_int,
                                                       int *__restrict__ nthr, int *__restrict__ status)
{
    extern __shared__ unsigned long long cum[];
    __shared__ unsigned long long part[256];
    __shared__ float pval[20];
    // cumulative histogram over v = 1..F (cum[0] = 0): per-thread chunks + serial fix-up
    const int per = (F + 256) / 256;
    const int v0 = threadIdx.x * per;
    unsigned long long s = 0;
    for (int v = v0; v < min(F + 1, v0 + per); v++) {
        s += v == 0 ? 0ull : hist[v];
        cum[v] = s;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < 64) {  // exclusive scan of the 256 chunk sums by one wave
        unsigned long long a0 = part[4 * threadIdx.x], a1 = part[4 * threadIdx.x + 1], a2 = part[4 * threadIdx.x + 2],
                           a3 = part[4 * threadIdx.x + 3];
        unsigned long long t = a0 + a1 + a2 + a3, x = t;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long y = __shfl_up(x, d, 64);
            if (static_cast<int>(threadIdx.x) >= d) x += y;
        }
        unsigned long long ex = x - t;
        part[4 * threadIdx.x] = ex;
        part[4 * threadIdx.x + 1] = ex + a0;
        part[4 * threadIdx.x + 2] = ex + a0 + a1;
        part[4 * threadIdx.x + 3] = ex + a0 + a1 + a2;
    }
    __syncthreads();
    for (int v = v0; v < min(F + 1, v0 + per); v++) cum[v] += part[threadIdx.x];
    __syncthreads();
    const unsigned long long n = cum[F];
    if (threadIdx.x < 20 && n > 0) {  // one percentile per lane: p = 95, 90, ..., 0
        const int p = 95 - 5 * static_cast<int>(threadIdx.x);
        const float nm1 = static_cast<float>(n - 1);
        const float q = __fdiv_rn(static_cast<float>(p), 100.0f);
        const float vi = __fmul_rn(nm1, q);
        long long prev, next;
        if (vi >= nm1) {
            prev = -1;
            next = -1;
        } else {
            prev = static_cast<long long>(floorf(vi));
            next = prev + 1;
            if (vi < 0.0f) prev = next = 0;
        }
        const unsigned long long ip = prev < 0 ? n - 1 : static_cast<unsigned long long>(prev);
        const unsigned long long in = next < 0 ? n - 1 : static_cast<unsigned long long>(next);
        const float gamma = static_cast<float>(static_cast<double>(vi) - static_cast<double>(prev));
        const float a = cum_order_stat(cum, F, ip);
        const float bb = cum_order_stat(cum, F, in);
        const float diff = __fsub_rn(bb, a);
        float r = __fadd_rn(a, __fmul_rn(diff, gamma));
        if (gamma >= 0.5f) r = __fsub_rn(bb, __fmul_rn(diff, __fsub_rn(1.0f, gamma)));
        pval[threadIdx.x] = r;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (n == 0) {
        *nthr = 0;
        *status = MC_ERR_EMPTY_OBSERVERS;
        return;
    }
    *status = MC_OK;
    int k = 0;
    for (int j = 0; j < 20; j++) {  // construction.py:88-95
        const int p = 95 - 5 * j;
        float r = pval[j];
        int isint = 0;
        if (r <= 1.0f) {
            if (p < 50) break;
            r = 1.0f;
            isint = 1;
        }
        thr[k] = r;
        is_int[k] = isint;
        k++;
    }
    *nthr = k;
}

}  // namespace mc
