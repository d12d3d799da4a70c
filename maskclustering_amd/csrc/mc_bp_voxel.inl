// mc_bp_voxel.inl — S1 back-projection, bp_launch_voxel: voxel_down_sample of every slot, in two LDS
// tiers and a global-hash kernel for what they hand on.
namespace mc {

// the slot's choice between bp_world and bp_world_affine, made once from the frame's K and pose (scalar
// loads: the same in every lane) and held in a scalar register, so that the branches on it are uniform
__device__ __forceinline__ bool bp_slot_affine(const double *__restrict__ K, const double *__restrict__ T, double trunc)
{
    return __builtin_amdgcn_readfirstlane(bp_pose_affine(K, T, trunc) ? 1 : 0) != 0;
}

// a slot's min-bound pass: the minimum of its pixels' world points per axis into mn (folded with mn's
// values on entry); NU pixels' loads per thread in flight.  Affine poses: the minimum of bp_world_lin and
// the translation added once by the caller (mc_bp_world.hpp).
template <bool kAffine, int T, int NU>
__device__ __forceinline__ void bp_min_pass(const double *__restrict__ K, const double *__restrict__ Tp,
                                            const double *rk, const unsigned *__restrict__ pl,
                                            const float *__restrict__ dep, int n, int W, int t, double mn[3])
{
    for (int k0 = t; k0 < n; k0 += NU * T) {
        unsigned iv[NU];
        float dv[NU];
#pragma unroll
        for (int u = 0; u < NU; u++) iv[u] = k0 + u * T < n ? pl[k0 + u * T] : 0u;
#pragma unroll
        for (int u = 0; u < NU; u++) dv[u] = k0 + u * T < n ? dep[iv[u]] : 0.f;
#pragma unroll
        for (int u = 0; u < NU; u++) {
            if (k0 + u * T < n) {
                double p[3];
                if (kAffine)
                    bp_world_lin(K, Tp, static_cast<int>(iv[u] % W), static_cast<int>(iv[u] / W), dv[u], p[0], p[1], p[2], rk);
                else
                    bp_world(K, Tp, static_cast<int>(iv[u] % W), static_cast<int>(iv[u] / W), dv[u], p[0], p[1], p[2], rk);
#pragma unroll
                for (int c = 0; c < 3; c++) mn[c] = fmin(mn[c], p[c]);
            }
        }
    }
}

// The two rules k_bp_voxel_lds and k_bp_voxel share, one definition each.
// A slot's min bound into mn, in every thread of the block of T: bp_min_pass by the slot's form, reduce(mn, mx)
// (the kernel's block min / max reduction; order-free), then an affine slot's translation once.  mn and mx
// hold DBL_MAX and -DBL_MAX on entry (the callers' initialisers: set here, the kernels compiled differently).
template <int T, int NU, typename Reduce>
__device__ __forceinline__ void bp_slot_min_bound(const double *__restrict__ K, const double *__restrict__ Tp,
                                                  const double *rk, const unsigned *__restrict__ pl,
                                                  const float *__restrict__ dep, int n, int W, int t, bool affine,
                                                  Reduce &&reduce, double mn[3], double mx[3])
{
    if (affine) bp_min_pass<true, T, NU>(K, Tp, rk, pl, dep, n, W, t, mn);
    else bp_min_pass<false, T, NU>(K, Tp, rk, pl, dep, n, W, t, mn);
    reduce(mn, mx);
    if (affine)  // (the translation once per slot: bp_min_pass)
#pragma unroll
        for (int c = 0; c < 3; c++) mn[c] = mn[c] + Tp[4 * c + 3];
}
// The slot's denoise grid origin: the voxel grid's (below every voxel mean: a mean of points >= the min
// bound), for k_bp_denoise_lds and k_bp_knn_ring
__device__ __forceinline__ void bp_store_grid_origin(double *__restrict__ slot_grid, int s, const double vmin[3])
{
#pragma unroll
    for (int c = 0; c < 3; c++) slot_grid[8 * static_cast<size_t>(s) + c] = vmin[c];
}

// ---------------------------------------------------------------------------------------------
// (a3) voxel_down_sample(0.01) (:105), workgroup per slot
// ---------------------------------------------------------------------------------------------
// Open3D: min bound - voxel/2, index = floor((p - vmin) / voxel), per-voxel sum in input order,
// mean = sum / count.  Output order (u2): first occurrence in pixel order.
// k_bp_voxel_lds (every slot, largest first), one workgroup per slot, the voxel hash in LDS:
//   0. min bound of the slot's world points (order-free block reduction; the points are not stored)
//   1. chunks of T pixels in list order, the next chunk's pixel and depth loads in flight under this
//      one; each pixel's world point is recomputed (bit for bit the one of 0.) and staged in LDS.
//      Runs of consecutive pixels with the same voxel key (within a wave) are found by comparing
//      every lane's key with the previous lane's: only a run's first pixel probes the hash.  The
//      chunk's first pixel of every voxel it touches is found by an LDS atomicMin of the thread id in
//      the voxel's hash entry; each run ORs its lanes into that thread's per-wave lane masks; new
//      voxels get ids in order of their first pixel (wave counts + prefix).  Then the chunk-first
//      thread of each voxel adds the voxel's pixels of this chunk, in pixel order (mask words in
//      wave order, bits ascending), to the voxel's running sum (global, loaded under the masks'
//      barrier).  Chunks run in order, so every voxel's sum is the left fold in input order that
//      Open3D's AccumulatedPoint makes, exactly.
//   2. a thread per voxel: mean = sum / count
// 0. and 1. compute the points by the affine form (no row 3 of the pose, no homogeneous divide) for a
// slot whose frame passes bp_pose_affine, by the general form otherwise: chosen once per slot, a uniform
// branch around two instantiations of each loop's point computation (mc_bp_world.hpp: the same bits).
// Three barriers per chunk, no per-pixel global stores.  A slot whose voxel coordinates span >= 1024
// voxels on an axis or that has more than V voxels is listed for the next tier (the larger LDS
// table, then k_bp_voxel, the global-hash kernel below).
// Largest slots first (their per-slot time grows with the pixel count): slots binned by
// floor(4 log2(pixels)) (the top three bits of the count), bins in descending order.  One workgroup.
__device__ __forceinline__ int vox_order_bin(int np)
{
    const unsigned x = static_cast<unsigned>(max(np, 1));
    const int b = 31 - __clz(x);
    return b < 2 ? b : 4 * b + static_cast<int>((x >> (b - 2)) & 3u) - 6;  // 0 .. 121, monotone in np
}
__global__ __launch_bounds__(1024) void k_bp_vox_order(const int *__restrict__ dNS, const int *__restrict__ slot_np,
                                                       int *__restrict__ order)
{
    constexpr int NB = 128;
    __shared__ int cnt[NB];
    const int NS = *dNS, t = threadIdx.x;
    if (t < NB) cnt[t] = 0;
    __syncthreads();
    for (int s = t; s < NS; s += 1024) atomicAdd(&cnt[vox_order_bin(slot_np[s])], 1);
    __syncthreads();
    if (t == 0) {
        int o = 0;
        for (int b = NB - 1; b >= 0; b--) {
            const int c = cnt[b];
            cnt[b] = o;
            o += c;
        }
    }
    __syncthreads();
    for (int s = t; s < NS; s += 1024) order[atomicAdd(&cnt[vox_order_bin(slot_np[s])], 1)] = s;
}


// tiers: <256, 2176, 2048> (31 KB of LDS, five workgroups per CU: the kernel waits on latency, and a
// fifth workgroup hides more of it than the 3072-entry table's shorter probes at high load save:
// C3 voxel 20.7 -> 19.8 ms per scene) for every slot; <512, 12288, 8192> (155 KB, one per CU; the
// running sums of a slot's first 512 voxels in LDS) for the slots the first tier lists; the
// global-hash kernel after that.  (Measured and not kept: the first 512 / 1408 voxels' running sums
// in LDS in the first tier at three / two workgroups per CU: 23.9 / 30.8 ms.)
constexpr int kVxT = 256, kVxH = 2176, kVxV = 2048;    // first tier: threads (pixels per chunk), hash entries, voxels
constexpr int kVxWpe = 5;                              // its waves per SIMD (= workgroups per CU)
constexpr int kVxT2 = 512, kVxH2 = 12288, kVxV2 = 8192, kVxL2 = 512;  // second tier (+ LDS running sums)
constexpr unsigned kVxEmpty = ~0u;

template <int T, int H, int V, int VL, int WPE = 1>
__global__ __launch_bounds__(T, WPE) void k_bp_voxel_lds(const int *__restrict__ dNS, const int *__restrict__ order,
                                                    const int *__restrict__ slot_frame, const int *__restrict__ slot_np,
                                                    const int *__restrict__ slot_pix,
                                                    const unsigned *__restrict__ pix_list, const float *__restrict__ depth,
                                                    const double *__restrict__ intr, const double *__restrict__ pose,
                                                    BpDev pr, int *__restrict__ vcnt, double *__restrict__ vpts,
                                                    int *__restrict__ slot_nv, int *__restrict__ fb_list,
                                                    int *__restrict__ fb_cnt, int force_fb, double *__restrict__ slot_grid)
{
    static_assert(T % 64 == 0 && T <= 1024 && V <= 0xFFFF, "chunk-first thread ids and voxel ids share 16 bits");
    constexpr int NW = T / 64;
    __shared__ unsigned hkey[H];
    __shared__ unsigned hval[H];                   // (voxel id << 16) | chunk-first thread (0xFFFF: none yet)
    __shared__ unsigned long long msk[T][NW];     // per chunk-first thread: its voxel's lanes of the chunk, by wave
    __shared__ double psx[T], psy[T], psz[T];     // the chunk's world points
    __shared__ double red[6 * NW];
    __shared__ int wsn[NW];
    __shared__ int s_flag;
    // the running sums of the slot's first VL voxels stay in LDS (no global round trip per chunk for
    // them); voxels numbered VL and up keep theirs at the slot's range of vpts / vcnt
    __shared__ double lsx[VL > 0 ? VL : 1], lsy[VL > 0 ? VL : 1], lsz[VL > 0 ? VL : 1];
    __shared__ int lcn[VL > 0 ? VL : 1];
    const int NS = *dNS;
    const int t = threadIdx.x, lane = lane_id(), wv = t >> 6;
    const int W = pr.W;
    const unsigned long long below = (1ull << lane) - 1ull;
#ifdef MC_BP_STAMPS
    unsigned long long stamp_prev = __builtin_amdgcn_s_memrealtime();
#endif
    for (int idx = blockIdx.x; idx < NS; idx += gridDim.x) {
        BP_STAMP(39);  // (the previous slot's means, 2.)
        const int s = order[idx];
        if (force_fb) {  // test knob: every slot to the global-hash kernel
            if (t == 0) fb_list[atomicAdd(fb_cnt, 1)] = s;
            continue;
        }
        const int f = slot_frame[s], n = slot_np[s], base = slot_pix[s];
        const double *K = intr + 4 * static_cast<size_t>(f);
        const double *Tp = pose + 16 * static_cast<size_t>(f);
        const float *dep = depth + static_cast<size_t>(f) * pr.H * W;
        const unsigned *pl = pix_list + base;
        double rk[2];
        bp_recip(K, rk);
        const bool affine = bp_slot_affine(K, Tp, pr.trunc);
        for (int i = t; i < H; i += T) {
            hkey[i] = kVxEmpty;
            hval[i] = ~0u;
        }
#pragma unroll
        for (int w = 0; w < NW; w++) msk[t][w] = 0ull;
        if (t == 0) s_flag = 0;
        // 0. min bound; four pixels' loads per thread in flight
        double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, mx[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
        bp_slot_min_bound<T, 4>(K, Tp, rk, pl, dep, n, W, t, affine,
                                [&](double *a, double *b) { block_minmax3_nw<NW>(a, b, red); }, mn, mx);
        BP_STAMP(36);  // 0. min bound
        double vmin[3];
#pragma unroll
        for (int c = 0; c < 3; c++) vmin[c] = uniform_d(mn[c] - pr.vs * 0.5);  // (scalar registers)
        if (t == 0) bp_store_grid_origin(slot_grid, s, vmin);
        // 1. chunks in list order: voxel ids in first-occurrence order and the running sums
        int nv = 0;
        unsigned ivA = t < n ? pl[t] : 0u;              // this chunk's pixel
        unsigned ivB = T + t < n ? pl[T + t] : 0u;      // the next chunk's
        float dA = t < n ? dep[ivA] : 0.f;
        asm volatile("" ::"v"(ivA), "v"(dA), "v"(ivB));  // (loaded before the loop: no wait at its head)
        for (int c0 = 0; c0 < n; c0 += T) {
            const int k = c0 + t;
            const bool valid = k < n;
            const unsigned iv = ivA;
            const float d = dA;
            unsigned key = kVxEmpty;
            if (valid) {
                double p[3];
                if (affine) bp_world_as<true>(K, Tp, static_cast<int>(iv % W), static_cast<int>(iv / W), d, p[0], p[1], p[2], rk);
                else bp_world_as<false>(K, Tp, static_cast<int>(iv % W), static_cast<int>(iv / W), d, p[0], p[1], p[2], rk);
                unsigned kk = 0;
                bool fits = true;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const double r = floor(div_rn(p[c] - vmin[c], pr.vs, pr.rvs));
                    fits = fits && r >= 0.0 && r < 1024.0;
                    kk = (kk << 10) | (fits ? static_cast<unsigned>(r) : 0u);
                }
                if (fits) key = kk;
                else s_flag = 1;
                psx[t] = p[0];
                psy[t] = p[1];
                psz[t] = p[2];
            }
            // runs: a lane whose key differs from the previous lane's starts one (invalid lanes, at
            // the end of the last chunk, and lanes that do not fit, which abandon the slot, start none)
            const unsigned prev = static_cast<unsigned>(__shfl_up(static_cast<int>(key), 1, 64));
            const bool head = key != kVxEmpty && (lane == 0 || prev != key);
            const unsigned long long ends = __ballot(head) | ~__ballot(key != kVxEmpty);
            int h = -1;
            unsigned long long run = 0ull;
            if (head) {
                const unsigned long long after = ends & ~(below | (1ull << lane));
                run = (after ? (after & (0ull - after)) - 1ull : ~0ull) & ~below;  // this lane .. the next run's first - 1
                unsigned e = mod_mul(key * 0x9E3779B1u, H);
                for (int probe = 0; probe < H; probe++) {
                    unsigned cur = hkey[e];
                    if (cur == kVxEmpty) {
                        cur = atomicCAS(&hkey[e], kVxEmpty, key);
                        if (cur == kVxEmpty) cur = key;
                    }
                    if (cur == key) {
                        h = static_cast<int>(e);
                        break;
                    }
                    e = e + 1 == static_cast<unsigned>(H) ? 0u : e + 1;
                }
                if (h < 0) s_flag = 1;
                else atomicMin(&hval[h], (hval[h] & 0xFFFF0000u) | static_cast<unsigned>(t));  // (the id half is stable here)
            }
            // the previous chunk's sums are stored before any thread loads them after the barrier (their
            // latency under this chunk's points and probes)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            // (the compiler's own wait for the next chunk's pixel lands here, where nothing is in flight,
            // not after the sums' loads below, where it would wait for them)
            asm volatile("" ::"v"(ivB));
            BP_STAMP(38);  // 1a. points, keys, runs, probes
            __syncthreads();  // hash entries, chunk-first threads, staged points
            if (s_flag) break;  // (uniform) overflow: the next tier takes the slot
            bool first = false, isnew = false;
            unsigned v = 0;
            if (h >= 0) {
                const unsigned hv = hval[h];
                const int tf = static_cast<int>(hv & 0xFFFFu);
                v = hv >> 16;
                first = tf == t;
                isnew = first && v == 0xFFFFu;
                atomicOr(&msk[tf][wv], run);
            }
            double ax = 0.0, ay = 0.0, az = 0.0;
            int cnt = 0;
            if (first && !isnew) {  // the running sum so far, loaded under the barrier
                if (v < static_cast<unsigned>(VL)) {
                    ax = lsx[v];
                    ay = lsy[v];
                    az = lsz[v];
                    cnt = lcn[v];
                } else {
                    const double *o = vpts + 3 * (static_cast<size_t>(base) + v);
                    ax = o[0];
                    ay = o[1];
                    az = o[2];
                    cnt = vcnt[base + v];
                }
            }
            // the next chunk's depths and the one after's pixels, behind the sums' loads (a wave's
            // memory operations complete in issue order: the fold waits for the sums only).  The
            // addresses are clamped rather than the loads skipped, so that both are always issued and
            // the compiler counts them (a conditional load makes its waits for the sums vmcnt(0)).
            ivA = ivB;
            dA = dep[k + T < n ? ivA : 0u];
            ivB = pl[min(k + 2 * T, n - 1)];
            const unsigned long long nm = __ballot(isnew);
            if (lane == 0) wsn[wv] = __popcll(nm);
            __syncthreads();  // every run's lanes in the masks, new voxels per wave
            // the prefetched depth and pixel (issued after the sums' loads, so this is the fold's wait
            // as well) arrive before the sums are stored: the stores, the chunk's last memory
            // operations, are then waited for only before the next barrier A, under the next chunk's
            // points and probes
            asm volatile("" ::"v"(dA), "v"(ivB));
            int tot = 0, before = 0;
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const int c = wsn[w];
                before += w < wv ? c : 0;
                tot += c;
            }
            if (isnew) {
                v = static_cast<unsigned>(nv + before + __popcll(nm & below));
                if (v >= static_cast<unsigned>(V)) s_flag = 1;
            }
            if (first && v < static_cast<unsigned>(V)) {
                // this chunk's pixels of voxel v, in pixel order, each pixel's staged point loaded one
                // pixel ahead of the adds (the same sums in the same order, the LDS latency under the
                // previous pixel's adds)
                unsigned long long mnext = msk[t][0];
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    unsigned long long m = mnext;
                    if (w + 1 < NW) mnext = msk[t][w + 1];  // the next wave's word under this one's adds
                    if (!m) continue;
                    msk[t][w] = 0ull;
                    cnt += __popcll(m);
                    int i = 64 * w + static_cast<int>(__builtin_ctzll(m));
                    m &= m - 1ull;
                    double cx = psx[i], cy = psy[i], cz = psz[i];
                    while (m) {
                        i = 64 * w + static_cast<int>(__builtin_ctzll(m));
                        m &= m - 1ull;
                        const double nx = psx[i], ny = psy[i], nz = psz[i];
                        ax = ax + cx;
                        ay = ay + cy;
                        az = az + cz;
                        cx = nx;
                        cy = ny;
                        cz = nz;
                    }
                    ax = ax + cx;
                    ay = ay + cy;
                    az = az + cz;
                }
                if (v < static_cast<unsigned>(VL)) {
                    lsx[v] = ax;
                    lsy[v] = ay;
                    lsz[v] = az;
                    lcn[v] = cnt;
                } else {
                    double *o = vpts + 3 * (static_cast<size_t>(base) + v);
                    o[0] = ax;
                    o[1] = ay;
                    o[2] = az;
                    vcnt[base + v] = cnt;
                }
                hval[h] = (v << 16) | 0xFFFFu;
            }
            nv += tot;
            BP_STAMP(40);  // 1b. masks, ids, ordered sums
            __syncthreads();  // staged points, masks and hash entries free for the next chunk
        }
        sync_global();  // the last chunk's sums, read by other threads in 2.
        if (s_flag) {  // (uniform) the global-hash kernel or the next tier takes the slot
            if (t == 0) fb_list[atomicAdd(fb_cnt, 1)] = s;
            __syncthreads();
            continue;
        }
        BP_STAMP(37);  // 1. ids and running sums
        // 2. means
        for (int v = t; v < nv; v += T) {
            double *o = vpts + 3 * (static_cast<size_t>(base) + v);
            if (v < VL) {
                const double dn = static_cast<double>(lcn[v]);
                o[0] = lsx[v] / dn;
                o[1] = lsy[v] / dn;
                o[2] = lsz[v] / dn;
            } else {
                const double dn = static_cast<double>(vcnt[base + v]);
                o[0] = o[0] / dn;
                o[1] = o[1] / dn;
                o[2] = o[2] / dn;
            }
        }
        if (t == 0) slot_nv[s] = nv;
        __syncthreads();
    }
}

// k_bp_voxel: the global-hash form for the slots k_bp_voxel_lds lists (voxel coordinates spanning
// >= 1024 voxels, or more than kVxV voxels).  Chunks of 256 pixels in list order: voxel keys go into
// the slot's hash (2 entries per pixel, empty at rest); new voxels get ids in order of their first
// pixel (atomicMin of the pixel rank, then an ordered scan); the sums are added wave by wave, lane
// by lane, i.e. in pixel order.
__global__ __launch_bounds__(256) void k_bp_voxel(const int *__restrict__ dNS, const int *__restrict__ order,
                                                  const int *__restrict__ slot_frame,
                                                  const int *__restrict__ slot_np, const int *__restrict__ slot_pix,
                                                  const unsigned *__restrict__ pix_list, const float *__restrict__ depth,
                                                  const double *__restrict__ intr, const double *__restrict__ pose, BpDev pr,
                                                  unsigned long long *__restrict__ hkey, int *__restrict__ hvid,
                                                  int *__restrict__ hfirst, int *__restrict__ vox_entry,
                                                  double *__restrict__ acc, double *__restrict__ vpts,
                                                  int *__restrict__ slot_nv, int *__restrict__ errflag,
                                                  double *__restrict__ slot_grid)
{
    __shared__ double sp[256 * 3];
    __shared__ double red[24];
    __shared__ int ws[4];
    const int NS = *dNS;
    const int t = threadIdx.x, lane = lane_id(), wv = t >> 6;
    const int W = pr.W;
    for (int idx = blockIdx.x; idx < NS; idx += gridDim.x) {
        const int s = order[idx];
        const int f = slot_frame[s], n = slot_np[s], base = slot_pix[s];
        const double *K = intr + 4 * static_cast<size_t>(f);
        const double *T = pose + 16 * static_cast<size_t>(f);
        const float *dep = depth + static_cast<size_t>(f) * pr.H * W;
        const unsigned *pl = pix_list + base;
        double rk[2];
        bp_recip(K, rk);
        const bool affine = bp_slot_affine(K, T, pr.trunc);
        // min bound (order-free)
        double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, mx[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
        bp_slot_min_bound<256, 1>(K, T, rk, pl, dep, n, W, t, affine,
                                  [&](double *a, double *b) { block_minmax3(a, b, red); }, mn, mx);
        double vmin[3];
#pragma unroll
        for (int c = 0; c < 3; c++) vmin[c] = mn[c] - pr.vs * 0.5;
        if (t == 0) bp_store_grid_origin(slot_grid, s, vmin);
        const unsigned C = 2u * static_cast<unsigned>(n);
        unsigned long long *hk = hkey + 2 * static_cast<size_t>(base);
        int *hv = hvid + 2 * static_cast<size_t>(base);
        int *hf = hfirst + 2 * static_cast<size_t>(base);
        double *ac = acc + 4 * static_cast<size_t>(base);
        int nv = 0;
        for (int c0 = 0; c0 < n; c0 += 256) {
            const int k = c0 + t;
            const bool valid = k < n;
            double p[3] = {0.0, 0.0, 0.0};
            unsigned e = 0;
            if (valid) {
                const unsigned i = pl[k];
                if (affine) bp_world_as<true>(K, T, static_cast<int>(i % W), static_cast<int>(i / W), dep[i], p[0], p[1], p[2], rk);
                else bp_world_as<false>(K, T, static_cast<int>(i % W), static_cast<int>(i / W), dep[i], p[0], p[1], p[2], rk);
                long long ix[3];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    ix[c] = static_cast<long long>(floor(div_rn(p[c] - vmin[c], pr.vs, pr.rvs)));
                    if (ix[c] < 0 || ix[c] >= (1ll << 21)) {
                        atomicOr(errflag, 1);
                        ix[c] = ix[c] < 0 ? 0 : (1ll << 21) - 1;
                    }
                }
                const unsigned long long key = pack3(static_cast<int>(ix[0]), static_cast<int>(ix[1]), static_cast<int>(ix[2]));
                e = mod_mul(bp_hash64(key), C);
                // bounded probe: the slot's 2n entries start empty (kept empty by the reset below)
                // and take <= n keys, so a free or matching entry exists; a table left dirty (a
                // broken invariant) ends in an error flag instead of a wave that never finishes
                for (unsigned probe = 0;; probe++) {
                    if (probe == C) {
                        atomicOr(errflag, 2);
                        break;
                    }
                    unsigned long long cur = hk[e];
                    if (cur == kEmptyKey) {
                        cur = atomicCAS(&hk[e], kEmptyKey, key);
                        if (cur == kEmptyKey) cur = key;
                    }
                    if (cur == key) break;
                    e = e + 1 == C ? 0 : e + 1;
                }
                if (ld_agent(&hv[e]) < 0) atomicMin(&hf[e], k);
            }
            sync_global();
            const bool first = valid && ld_agent(&hv[e]) < 0 && ld_agent(&hf[e]) == k;
            int tot;
            const int pos = block_excl_scan<256>(first ? 1 : 0, ws, tot);
            if (first) {
                const int v = nv + pos;
                st_agent(&hv[e], v);
                vox_entry[base + v] = static_cast<int>(e);
                ac[4 * v] = 0.0;
                ac[4 * v + 1] = 0.0;
                ac[4 * v + 2] = 0.0;
                ac[4 * v + 3] = 0.0;
            }
            sync_global();
            const int vid = valid ? ld_agent(&hv[e]) : -1;
            sp[3 * t] = p[0];
            sp[3 * t + 1] = p[1];
            sp[3 * t + 2] = p[2];
            sync_global();
            // group lanes by voxel (ballots only), then every group leader of the wave adds its
            // group's points in lane order to the running sum at once (one round trip per wave)
            unsigned long long gm = 0;
            {
                unsigned long long act = __ballot(vid >= 0);
                while (act) {
                    const int L = __ffsll(static_cast<long long>(act)) - 1;
                    const int kk = __shfl(vid, L, 64);
                    const unsigned long long m = __ballot(vid == kk);
                    if (lane == L) gm = m;
                    act &= ~m;
                }
            }
#pragma unroll
            for (int w = 0; w < 4; w++) {
                if (wv == w && gm) {  // AccumulatedPoint::AddPoint, lane (= pixel) order
                    double ax = ac[4 * vid], ay = ac[4 * vid + 1], az = ac[4 * vid + 2], an = ac[4 * vid + 3];
                    unsigned long long mm = gm;
                    while (mm) {
                        const int l = __ffsll(static_cast<long long>(mm)) - 1;
                        mm &= mm - 1;
                        const double *q = sp + 3 * (w * 64 + l);
                        ax = ax + q[0];
                        ay = ay + q[1];
                        az = az + q[2];
                        an = an + 1.0;
                    }
                    ac[4 * vid] = ax;
                    ac[4 * vid + 1] = ay;
                    ac[4 * vid + 2] = az;
                    ac[4 * vid + 3] = an;
                }
                sync_global();
            }
            nv += tot;
        }
        // means; the hash entries of this slot return to empty
        for (int v = t; v < nv; v += 256) {
            const double cnt = ac[4 * v + 3];
            vpts[3 * (static_cast<size_t>(base) + v)] = ac[4 * v] / cnt;
            vpts[3 * (static_cast<size_t>(base) + v) + 1] = ac[4 * v + 1] / cnt;
            vpts[3 * (static_cast<size_t>(base) + v) + 2] = ac[4 * v + 2] / cnt;
            const int e = vox_entry[base + v];
            hk[e] = kEmptyKey;
            st_agent(&hv[e], -1);
            st_agent(&hf[e], INT_MAX);
        }
        if (t == 0) slot_nv[s] = nv;
        sync_global();
    }
}

}  // namespace mc
