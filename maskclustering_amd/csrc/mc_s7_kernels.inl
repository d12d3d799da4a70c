// mc_s7_kernels.inl — S7 final point sets; included by mc_kernels.inl.  Launched by s7_ranges and s7_points
// (mc_cluster_host.inl).
// Final point sets: union of the member masks' point sets (node.py:35) as per-object
// bitmaps over each object's [min, max] point range, extracted in ascending order.
// Graph path: one thread per scene point, objects of the point from its mask list,
// wave-aggregated atomics (consecutive points of one object share a word).
namespace mc {

constexpr int kMaxObjPerPoint = 8;

// object of every global mask (-1: under-segmented, not a node)
__global__ __launch_bounds__(256) void k7_obj_of_mask(int M, const int *__restrict__ node_of_mask,
                                                      const int *__restrict__ final_label, int *__restrict__ obj)
{
    for (int g = blockIdx.x * 256 + threadIdx.x; g < M; g += gridDim.x * 256) {
        const int nd = node_of_mask[g];
        obj[g] = nd < 0 ? -1 : final_label[nd];
    }
}

// distinct objects of point p (from its mask list); returns count (-1 if more than cap)
__device__ __forceinline__ int point_objects(const int *pt_off, const unsigned *pt_list, const int *frame_start,
                                             const int *obj_of_mask, int p, int *objs)
{
    int n = 0;
    const int b = pt_off[p], e = pt_off[p + 1];
    for (int i = b; i < e; i++) {
        const unsigned en = pt_list[i];
        const int g = frame_start[en >> kLocalBits] + static_cast<int>(en & (kMaxMasksPerFrame - 1));
        const int k = obj_of_mask[g];
        if (k < 0) continue;
        bool seen = false;
        for (int j = 0; j < n; j++) seen |= objs[j] == k;
        if (seen) continue;
        if (n == kMaxObjPerPoint) return -1;
        objs[n++] = k;
    }
    return n;
}

// mode 0: per-object min/max point; mode 1: set bits
template <int MODE>
__global__ __launch_bounds__(256) void k7p_points(int P, const int *__restrict__ pt_off, const unsigned *__restrict__ pt_list,
                                                  const int *__restrict__ frame_start, const int *__restrict__ obj_of_mask,
                                                  int *__restrict__ pmin,
                                                  int *__restrict__ pmax, const int *__restrict__ woff,
                                                  unsigned long long *__restrict__ bm, int *__restrict__ overflow)
{
    const int lane = lane_id();
    const int p0 = (blockIdx.x * 256 + threadIdx.x) & ~63;
    const int p = p0 + lane;
    int objs[kMaxObjPerPoint];
    int n = 0;
    if (p < P) {
        n = point_objects(pt_off, pt_list, frame_start, obj_of_mask, p, objs);
        if (n < 0) {
            atomicOr(overflow, 1);
            n = 0;
        }
    }
    int nmax = n;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nmax = max(nmax, __shfl_xor(nmax, d, 64));
    for (int j = 0; j < nmax; j++) {
        int kk = j < n ? objs[j] : -1;
        while (true) {
            const unsigned long long act = __ballot(kk >= 0);
            if (!act) break;
            const int leader = __ffsll(static_cast<long long>(act)) - 1;
            const int K = __shfl(kk, leader, 64);
            const unsigned long long m = __ballot(kk == K);
            if (MODE == 0) {
                if (lane == leader) {
                    const int lo = __ffsll(static_cast<long long>(m)) - 1;
                    const int hi = 63 - __clzll(static_cast<long long>(m));
                    atomicMin(&pmin[K], p0 + lo);
                    atomicMax(&pmax[K], p0 + hi);
                }
            } else {
                const int base = pmin[K];  // wave-uniform load
                const long long off0 = static_cast<long long>(p0) - base;  // bit of lane 0
                // lanes of m span at most two 64-bit words
                const long long wlo = (off0 + (__ffsll(static_cast<long long>(m)) - 1)) >> 6;
                const long long whi = (off0 + (63 - __clzll(static_cast<long long>(m)))) >> 6;
                if (lane == leader) {
                    for (long long w = wlo; w <= whi; w++) {
                        const long long sh = off0 - 64 * w;  // bit of lane l in word w = sh + l
                        unsigned long long bits;
                        if (sh >= 0) bits = sh >= 64 ? 0ull : (m << sh);
                        else bits = -sh >= 64 ? 0ull : (m >> (-sh));
                        if (bits) atomicOr(&bm[woff[K] + w], bits);
                    }
                }
            }
            if (kk == K) kk = -1;
        }
    }
}

// general path (arbitrary level-0 nodes): wave per level-0 node
__global__ __launch_bounds__(256) void k7_minmax(int N0, const int *__restrict__ final_label,
                                                 const int *__restrict__ ptoff, const int *__restrict__ ptlen,
                                                 const int *__restrict__ pts, int *__restrict__ pmin,
                                                 int *__restrict__ pmax)
{
    const int lane = lane_id();
    for (int i = (blockIdx.x * 256 + threadIdx.x) >> 6; i < N0; i += gridDim.x * 4) {
        const int k = final_label[i];
        const int o = ptoff[i], l = ptlen[i];
        int mn = INT_MAX, mx = -1;
        for (int x = lane; x < l; x += 64) {
            const int p = pts[o + x];
            mn = min(mn, p);
            mx = max(mx, p);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            mn = min(mn, __shfl_xor(mn, d, 64));
            mx = max(mx, __shfl_xor(mx, d, 64));
        }
        if (lane == 0 && mx >= 0) {
            atomicMin(&pmin[k], mn);
            atomicMax(&pmax[k], mx);
        }
    }
}

__global__ __launch_bounds__(256) void k7_setbits(int N0, const int *__restrict__ final_label,
                                                  const int *__restrict__ ptoff, const int *__restrict__ ptlen,
                                                  const int *__restrict__ pts, const int *__restrict__ pmin,
                                                  const int *__restrict__ woff, unsigned long long *__restrict__ bm)
{
    const int lane = lane_id();
    for (int i = (blockIdx.x * 256 + threadIdx.x) >> 6; i < N0; i += gridDim.x * 4) {
        const int k = final_label[i];
        const int o = ptoff[i], l = ptlen[i];
        const int base = pmin[k];
        unsigned long long *row = bm + woff[k];
        for (int x0 = 0; x0 < l; x0 += 64) {
            const int x = x0 + lane;
            int w = -1;
            unsigned long long bit = 0;
            if (x < l) {
                const int q = pts[o + x] - base;
                w = q >> 6;
                bit = 1ull << (q & 63);
            }
            // combine lanes that hit the same word
            while (true) {
                const unsigned long long act = __ballot(w >= 0);
                if (!act) break;
                const int leader = __ffsll(static_cast<long long>(act)) - 1;
                const int W = __shfl(w, leader, 64);
                unsigned long long v = (w == W) ? bit : 0ull;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) v |= __shfl_xor(v, d, 64);
                if (lane == leader) atomicOr(&row[W], v);
                if (w == W) w = -1;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k7_words(const int *__restrict__ dK, const int *__restrict__ pmin,
                                                const int *__restrict__ pmax, int *__restrict__ nwords,
                                                int *__restrict__ stat_k)
{
    const int K = *dK;
    if (blockIdx.x == 0 && threadIdx.x == 0) *stat_k = K;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256)
        nwords[k] = pmax[k] >= pmin[k] ? ((pmax[k] - pmin[k]) >> 6) + 1 : 0;
}

__global__ __launch_bounds__(256) void k7_count(const int *__restrict__ dK, const int *__restrict__ woff,
                                                const unsigned long long *__restrict__ bm, int *__restrict__ ptcnt)
{
    __shared__ int ws[4];
    const int K = *dK;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        int s = 0;
        for (int w = woff[k] + threadIdx.x; w < woff[k + 1]; w += 256) s += __popcll(bm[w]);
        s = block_sum<256>(s, ws);
        if (threadIdx.x == 0) ptcnt[k] = s;
    }
}

__global__ __launch_bounds__(256) void k7_extract(const int *__restrict__ dK, const int *__restrict__ woff,
                                                  const unsigned long long *__restrict__ bm,
                                                  const int *__restrict__ pmin, const int *__restrict__ ptoff_out,
                                                  int *__restrict__ pts_out)
{
    __shared__ int ws[4];
    const int K = *dK;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const int wb = woff[k], we = woff[k + 1];
        const int RW = we - wb;
        const int per = (RW + 255) / 256;
        const int w0 = threadIdx.x * per, w1 = min(RW, w0 + per);
        int mine = 0;
        for (int w = w0; w < w1; w++) mine += __popcll(bm[wb + w]);
        int tot;
        int pos = block_excl_scan<256>(mine, ws, tot) + ptoff_out[k];
        const int base = pmin[k];
        for (int w = w0; w < w1; w++) {
            unsigned long long v = bm[wb + w];
            while (v) {
                const int bt = __ffsll(static_cast<long long>(v)) - 1;
                v &= v - 1;
                pts_out[pos++] = base + (w << 6) + bt;
            }
        }
    }
}

// pmin/pmax reset for up to n objects + zero a word range [0, *dwords) (grid-stride)
__global__ __launch_bounds__(256) void k7_reset(int n, int *__restrict__ pmin, int *__restrict__ pmax)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        pmin[i] = INT_MAX;
        pmax[i] = -1;
    }
}

__global__ void k_copy_i32(const int *src, int *dst) { *dst = *src; }

}  // namespace mc
