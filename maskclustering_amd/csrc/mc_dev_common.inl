// mc_dev_common.inl — device helpers that every kernel file of the library uses (included by mc_kernels.inl,
// first): ordering of LDS and global hand-offs inside a workgroup (wave_sync, sync_global), wave scans and
// reductions, the block-wide exclusive scan, device-scope loads and stores (ld_agent, st_agent), lane_id, and
// the spread counters (kSpread slots per counter; the host sizes d_spread and d_edges by them).
namespace mc {

// Orders LDS accesses between the lanes of one wave (a wave executes in lockstep; this
// keeps the compiler from moving LDS loads/stores across the point).
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int wave_incl_scan(int x)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

__device__ __forceinline__ int wave_sum(int x)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

__device__ __forceinline__ int wave_min_i(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// Workgroup barrier for data handed between waves through GLOBAL memory.  On gfx950 __syncthreads()
// is s_waitcnt lgkmcnt(0) + s_barrier: a plain global store (or a no-return atomic) of one wave can
// still be in flight when another wave loads the address after the barrier.  Every wave first waits
// for its own vector-memory operations (MI355X_MICROARCH.md: intra-workgroup hand-off through memory).
__device__ __forceinline__ void sync_global()
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// Block-wide exclusive scan for blockDim.x == NT (multiple of 64). `ws` holds NT/64 ints.
// (ev_block_scan, mc_ap_kernels.inl, restates it.)
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int *ws, int &total)
{
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = wave_incl_scan(v);
    if (lane == 63) ws[w] = x;
    __syncthreads();
    if (w == 0) {
        int s = lane < NW ? ws[lane] : 0;
        s = wave_incl_scan(s);
        if (lane < NW) ws[lane] = s;
    }
    __syncthreads();
    int base = w > 0 ? ws[w - 1] : 0;
    total = ws[NW - 1];
    __syncthreads();
    return base + x - v;
}

template <int NT>
__device__ __forceinline__ int block_sum(int v, int *ws)
{
    int t;
    block_excl_scan<NT>(v, ws, t);
    return t;
}

__device__ __forceinline__ int ld_agent(const int *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(int *p, int v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// Counters that many workgroups add to: one atomic on a single address serialises at its L2
// channel (~10 ns each, measured: 8192 waves -> ~90 us), so adds go to one of kSpread slots
// 128 B apart, picked by workgroup, and the reader folds the slots.
constexpr int kSpread = 64;
constexpr int kSpreadStrideI = 32;   // ints
constexpr int kSpreadStrideL = 16;   // u64
__device__ __forceinline__ void spread_add(int *base, int v)
{
    atomicAdd(base + (blockIdx.x & (kSpread - 1)) * kSpreadStrideI, v);
}
__device__ __forceinline__ void spread_add(unsigned long long *base, unsigned long long v)
{
    atomicAdd(base + (blockIdx.x & (kSpread - 1)) * kSpreadStrideL, v);
}

}  // namespace mc
