// mc_bp_common.inl — S1 back-projection: what every step of bp_run's kernels shares (included by
// mc_bp_kernels.inl): the step clocks of the stamps build, the cell hashes and keys, the ordered
// insert, a lane-uniform double in scalar registers, and the wave and block min / max reductions.
namespace mc {

// Diagnostic build only (-DMC_BP_STAMPS): per-step real-time-clock (100 MHz) totals of the S1 kernels' steps, summed
// over slots by thread 0 of every workgroup (shares, not durations: DESIGN.md §4).
#ifdef MC_BP_STAMPS
__device__ unsigned long long g_bp_stamps[48];
__device__ unsigned g_bp_slot_time[1 << 16];  // per-slot busy time (10 ns ticks), last batch
#define BP_STAMP(k)                                                                      \
    do {                                                                                 \
        __syncthreads();                                                                 \
        if (threadIdx.x == 0) {                                                          \
            const unsigned long long now_ = __builtin_amdgcn_s_memrealtime();                \
            atomicAdd(&g_bp_stamps[k], now_ - stamp_prev);                               \
            stamp_prev = now_;                                                           \
        }                                                                                \
    } while (0)
// the k-NN list pass's selected set of a point (0: deferred): [33] its sum over points, [31] the sum over
// waves of the wave's largest, [32] the waves (the pass runs as long as the lane with the largest set).
// Counted only with -DMC_BP_STAMPS_SEL beside -DMC_BP_STAMPS: the wave maximum costs the pass about as much
// as the pass itself, so the build that counts is not the build that times.
__device__ __forceinline__ void bp_stamp_selected(int sel)
{
    atomicAdd(&g_bp_stamps[33], static_cast<unsigned long long>(sel));
    unsigned long long act = __ballot(1);
    const int first = __ffsll(static_cast<long long>(act)) - 1;
    int mx = 0;
    while (act) {
        mx = max(mx, __shfl(sel, __ffsll(static_cast<long long>(act)) - 1, 64));
        act &= act - 1;
    }
    if (static_cast<int>(threadIdx.x & 63u) == first) {
        atomicAdd(&g_bp_stamps[31], static_cast<unsigned long long>(mx));
        atomicAdd(&g_bp_stamps[32], 1ull);
    }
}
#else
#define BP_STAMP(k) do { } while (0)
#endif

// cell hash for the hashed grids (bucket = mod_mul(hash, buckets), i.e. the hash's high bits): a
// linear form with odd golden-ratio-like multipliers (three multiply-adds; the walks hash up to 27
// cells per point, so the hash is on their critical path); the buckets only need cells spread out,
// the key test separates the cells a bucket shares
__device__ __forceinline__ unsigned bp_hash3(int x, int y, int z)
{
    return static_cast<unsigned>(x) * 0x9E3779B1u + static_cast<unsigned>(y) * 0x85EBCA77u +
           static_cast<unsigned>(z) * 0xC2B2AE3Du;
}
__device__ __forceinline__ unsigned bp_hash64(unsigned long long k)
{
    k *= 0x9E3779B97F4A7C15ull;
    return static_cast<unsigned>(k >> 32) ^ static_cast<unsigned>(k);
}
// h mod n without a division
__device__ __forceinline__ unsigned mod_mul(unsigned h, unsigned n)
{
    return static_cast<unsigned>((static_cast<unsigned long long>(h) * n) >> 32);
}
__device__ __forceinline__ unsigned long long pack3(int x, int y, int z)
{
    return (static_cast<unsigned long long>(x) << 42) | (static_cast<unsigned long long>(y) << 21) |
           static_cast<unsigned long long>(z);
}

__device__ __forceinline__ void unpack3(unsigned long long k, int &x, int &y, int &z)
{
    x = static_cast<int>((k >> 42) & 0x1FFFFF);
    y = static_cast<int>((k >> 21) & 0x1FFFFF);
    z = static_cast<int>(k & 0x1FFFFF);
}
// scene_cell (the 2r scene grid's cell coordinate) and kCellBias: mc_bp_qcell.hpp

// div_rn (a / b from RN(1 / b): a multiply and two FMAs instead of the division sequence v_rcp_f64, scale,
// five FMAs, fixup; the same bits as a / b), bp_recip, and the world point of a pixel in its general and
// affine forms (bp_world, bp_world_affine, bp_pose_affine): mc_bp_world.hpp.  S1's per-pixel divisions
// are div_rn's: the unprojection by fx and fy, and the voxel index by the voxel size.

// (a1, u1): Open3D create_from_depth_image + transform, in double, no FMA
// floor(a / b) of the cell indices (the denoise's grid; per voxel, not per pixel)
__device__ __forceinline__ double floor_div(double a, double b) { return floor(a / b); }

// a value equal in every lane, moved to scalar registers (frees its VGPRs for the rest of the slot)
__device__ __forceinline__ double uniform_d(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readfirstlane(static_cast<int>(b & 0xFFFFFFFFll));
    const int hi = __builtin_amdgcn_readfirstlane(static_cast<int>(b >> 32));
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
}

// (u3): nanoflann L2 for 3-D, ((dx*dx + dy*dy) + dz*dz)
__device__ __forceinline__ double bp_d2(const double *a, const double *b)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

__device__ __forceinline__ double wave_min_d(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ double wave_max_d(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}

// block (256) min / max of 3 doubles, broadcast to every thread; red holds 2*3*4 doubles
// (pp_block_minmax3, mc_pp_kernels.inl, restates it for NT threads)
__device__ __forceinline__ void block_minmax3(double mn[3], double mx[3], double *red)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double a = wave_min_d(mn[c]), b = wave_max_d(mx[c]);
        if (lane == 0) {
            red[c * 4 + wv] = a;
            red[12 + c * 4 + wv] = b;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; c++) {
        mn[c] = fmin(fmin(red[c * 4], red[c * 4 + 1]), fmin(red[c * 4 + 2], red[c * 4 + 3]));
        mx[c] = fmax(fmax(red[12 + c * 4], red[12 + c * 4 + 1]), fmax(red[12 + c * 4 + 2], red[12 + c * 4 + 3]));
    }
    __syncthreads();
}

template <int NW>
__device__ __forceinline__ void block_minmax3_nw(double mn[3], double mx[3], double *red)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double a = wave_min_d(mn[c]), b = wave_max_d(mx[c]);
        if (lane == 0) {
            red[c * NW + wv] = a;
            red[3 * NW + c * NW + wv] = b;
        }
    }
    __syncthreads();
    // the NW partials of each component across the lanes of every wave, then a wave reduction (not
    // 6 * NW values per lane: unrolled, those spilled to scratch in the 16-wave classes)
#pragma unroll
    for (int c = 0; c < 3; c++) {
        mn[c] = wave_min_d(lane < NW ? red[c * NW + lane] : DBL_MAX);
        mx[c] = wave_max_d(lane < NW ? red[3 * NW + c * NW + lane] : -DBL_MAX);
    }
    __syncthreads();
}

// sorted insert of v into the ascending array a[0..N) (drops the largest): new a[q] =
// min(a[q], max(a[q-1], v)) (a[q-1] if v < a[q-1], v if a[q-1] <= v < a[q], else a[q]), two native
// min / max operations per step instead of two compares and four selects (no NaN reaches here:
// squared distances and DBL_MAX / INT_MAX sentinels)
__device__ __forceinline__ double ins_min(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ double ins_max(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ int ins_min(int a, int b) { return min(a, b); }
__device__ __forceinline__ int ins_max(int a, int b) { return max(a, b); }
template <int N, typename V>
__device__ __forceinline__ void sorted_insert(V (&a)[N], V v)
{
    if (!(v < a[N - 1])) return;
#pragma unroll
    for (int q = N - 1; q > 0; q--) a[q] = ins_min(a[q], ins_max(a[q - 1], v));
    a[0] = ins_min(a[0], v);
}

}  // namespace mc
