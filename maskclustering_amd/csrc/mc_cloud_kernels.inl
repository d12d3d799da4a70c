// mc_cloud_kernels.inl — kernels of the scene point cloud fusion (mc_cloud_*; host: mc_cloud_host.inl, decisions and
// shared rules: mc_cloud_plan.hpp; tasmap/tasmap2mct_format.py:216-284).
//
// A stage is one voxel_down_sample of n points, chip-wide and in input order:
//   input    k_cloud_frame_prep, k_cloud_count, (scan), k_cloud_compact: the valid pixels of a buffer's frames,
//            frame-major then row-major, as world points (mc_bp_world.hpp, S1's arithmetic) and colour bytes
//   bounds   k_cloud_bounds, k_cloud_bounds_final: per-axis minimum and maximum (order-free), a non-finite flag
//   hash     k_cloud_insert: the packed voxel key of every point into an open-addressing table; per entry
//            the population and the smallest point index.  Atomics place integers only.
//   order    k_cloud_flag, (scan), k_cloud_voxels: a voxel's number is the count of first points before its
//            own first point: first-occurrence order without a sort
//   lists    (scan), k_cloud_scatter: the voxels' point lists, unordered (atomic cursors)
//   fold     k_cloud_fold_small / k_cloud_fold_block: per voxel the list in ascending index order, then the
//            left fold of points and colours in float64 and the division by the population.  One thread
//            folds one channel, so the order of the additions is the input order whatever ran first.
// No product feeds a sum through a fused multiply-add (the library is built with -ffp-contract=off).
namespace mc {

constexpr int kCloudNone = 0, kCloudU8 = 1, kCloudF64 = 2;  // the colours of a stage's input

// per frame: whether the affine pose form gives the general form's bits (bp_pose_affine), and RN(1/fx), RN(1/fy)
__global__ __launch_bounds__(64) void k_cloud_frame_prep(int F, const double *__restrict__ K, const double *__restrict__ T,
                                                         double trunc, int *__restrict__ affine, double *__restrict__ rk)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= F) return;
    affine[f] = bp_pose_affine(K + 4 * f, T + 16 * f, trunc) ? 1 : 0;
    bp_recip(K + 4 * f, rk + 2 * f);
}

__device__ __forceinline__ bool cloud_valid(float d, double trunc)
{
    return d > 0.f && static_cast<double>(d) < trunc;  // false for NaN; +inf and d == trunc are dropped
}

// valid pixels of each tile of kCloudTilePx pixels
__global__ __launch_bounds__(256) void k_cloud_count(const float *__restrict__ depth, int64_t npx, double trunc,
                                                     int *__restrict__ tile_cnt)
{
    __shared__ int ws[4];
    const int64_t p0 = static_cast<int64_t>(blockIdx.x) * kCloudTilePx + threadIdx.x * 4;
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (p0 + k < npx && cloud_valid(depth[p0 + k], trunc)) c++;
    c = block_sum<256>(c, ws);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = c;
}

// the valid pixels' world points and colour bytes, in pixel order, from tile_off[tile] on
__global__ __launch_bounds__(256) void k_cloud_compact(const float *__restrict__ depth, const unsigned char *__restrict__ rgb,
                                                       int64_t npx, int H, int W, const double *__restrict__ K,
                                                       const double *__restrict__ T, const int *__restrict__ affine,
                                                       const double *__restrict__ rk, double trunc,
                                                       const int *__restrict__ tile_off, double *__restrict__ pts,
                                                       unsigned char *__restrict__ col)
{
    __shared__ int ws[4];
    const int64_t p0 = static_cast<int64_t>(blockIdx.x) * kCloudTilePx + threadIdx.x * 4;
    float d[4];
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        d[k] = p0 + k < npx ? depth[p0 + k] : 0.f;
        if (cloud_valid(d[k], trunc)) c++;
    }
    int tot;
    int64_t o = static_cast<int64_t>(tile_off[blockIdx.x]) + block_excl_scan<256>(c, ws, tot);
    const int64_t hw = static_cast<int64_t>(H) * W;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (!cloud_valid(d[k], trunc)) continue;
        const int64_t p = p0 + k;
        const int f = static_cast<int>(p / hw);
        const int r = static_cast<int>(p - f * hw);
        const int v = r / W, u = r - v * W;
        double x, y, z;
        if (affine[f]) bp_world_affine(K + 4 * f, T + 16 * f, u, v, d[k], x, y, z, rk + 2 * f);
        else bp_world(K + 4 * f, T + 16 * f, u, v, d[k], x, y, z, rk + 2 * f);
        pts[3 * o] = x, pts[3 * o + 1] = y, pts[3 * o + 2] = z;
        col[3 * o] = rgb[3 * p], col[3 * o + 1] = rgb[3 * p + 1], col[3 * o + 2] = rgb[3 * p + 2];
        o++;
    }
}

__device__ __forceinline__ double cloud_wave_min(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ double cloud_wave_max(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}

// a 256-thread workgroup's minimum and maximum of three axes into out[0..2], out[3..5] (thread 0 writes)
__device__ __forceinline__ void cloud_block_bounds(double mn[3], double mx[3], double *out)
{
    __shared__ double sh[4][6];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        mn[r] = cloud_wave_min(mn[r]);
        mx[r] = cloud_wave_max(mx[r]);
    }
    if (lane == 0)
        for (int r = 0; r < 3; r++) sh[w][r] = mn[r], sh[w][3 + r] = mx[r];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int r = 0; r < 3; r++) {
            out[r] = fmin(fmin(sh[0][r], sh[1][r]), fmin(sh[2][r], sh[3][r]));
            out[3 + r] = fmax(fmax(sh[0][3 + r], sh[1][3 + r]), fmax(sh[2][3 + r], sh[3][3 + r]));
        }
}

// per workgroup the bounds of its points (grid-stride); flag[0] |= 1 when a coordinate is NaN or infinite
__global__ __launch_bounds__(256) void k_cloud_bounds(const double *__restrict__ pts, int64_t n, double *__restrict__ partial,
                                                      int *__restrict__ flag)
{
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256)
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double x = pts[3 * i + r];
            bad = bad || !(fabs(x) <= 1.7976931348623157e308);
            mn[r] = fmin(mn[r], x);
            mx[r] = fmax(mx[r], x);
        }
    if (bad) atomicOr(flag, 1);
    cloud_block_bounds(mn, mx, partial + 6 * blockIdx.x);
}

__global__ __launch_bounds__(256) void k_cloud_bounds_final(const double *__restrict__ partial, int nb, double *__restrict__ out)
{
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < nb; b += 256)
#pragma unroll
        for (int r = 0; r < 3; r++) {
            mn[r] = fmin(mn[r], partial[6 * b + r]);
            mx[r] = fmax(mx[r], partial[6 * b + 3 + r]);
        }
    cloud_block_bounds(mn, mx, out);
}

// Every point's key into the table (linear probing from cloud_hash; the table has at least two entries a
// point, so a free entry is met).  bounds[0..2] is the stage's minimum; the host has checked that every
// index is below 2^21 (cloud_check_extent).  slot_of[i] is the entry of point i's voxel.
__global__ __launch_bounds__(256) void k_cloud_insert(const double *__restrict__ pts, int64_t n, const double *__restrict__ bounds,
                                                      double voxel, unsigned long long *__restrict__ tab, int log2_table,
                                                      int *__restrict__ cnt, unsigned *__restrict__ first,
                                                      unsigned *__restrict__ slot_of)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t mask = (uint64_t(1) << log2_table) - 1;
    int64_t ix[3];
#pragma unroll
    for (int r = 0; r < 3; r++) ix[r] = cloud_voxel_index(pts[3 * i + r], cloud_vmin(bounds[r], voxel), voxel) & (kCloudMaxAxis - 1);
    const unsigned long long key = cloud_pack_key(ix[0], ix[1], ix[2]);
    uint64_t s = cloud_hash(key, log2_table) & mask;
    for (uint64_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
        unsigned long long cur = tab[s];
        if (cur == kCloudEmptyKey) cur = atomicCAS(&tab[s], static_cast<unsigned long long>(kCloudEmptyKey), key);
        if (cur == kCloudEmptyKey || cur == key) {
            atomicAdd(&cnt[s], 1);
            atomicMin(&first[s], static_cast<unsigned>(i));
            slot_of[i] = static_cast<unsigned>(s);
            return;
        }
    }
    slot_of[i] = 0;  // (not reached: the table is never full)
}

// flag[i] = 1 where point i is the first of its voxel
__global__ __launch_bounds__(256) void k_cloud_flag(int64_t n, const unsigned *__restrict__ slot_of,
                                                    const unsigned *__restrict__ first, int *__restrict__ flag)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) flag[i] = first[slot_of[i]] == static_cast<unsigned>(i) ? 1 : 0;
}

// a voxel's first point hands the voxel its number: the population to vcnt[number], the number into the
// table entry's count word (read from here on as "voxel of the entry"), the largest population to *maxpop
__global__ __launch_bounds__(256) void k_cloud_voxels(int64_t n, const int *__restrict__ flag, const int *__restrict__ vnum,
                                                      const unsigned *__restrict__ slot_of, int *__restrict__ cnt,
                                                      int *__restrict__ vcnt, int *__restrict__ maxpop)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    int c = 0;
    if (i < n && flag[i]) {
        const unsigned s = slot_of[i];
        c = cnt[s];
        vcnt[vnum[i]] = c;
        cnt[s] = vnum[i];
    }
    c = wave_max_i(c);
    if (lane_id() == 0 && c > 0) atomicMax(maxpop, c);
}

__global__ __launch_bounds__(256) void k_cloud_scatter(int64_t n, const unsigned *__restrict__ slot_of,
                                                       const int *__restrict__ vox_of_slot, const int *__restrict__ voff,
                                                       int *__restrict__ cursor, int *__restrict__ list)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const int v = vox_of_slot[slot_of[i]];
    const int pos = voff[v] + atomicAdd(&cursor[v], 1);
    list[pos] = static_cast<int>(i);
}

// channel ch (0..2 point, 3..5 colour) of point p as the fold adds it; a colour byte is divided here
template <int kCol>
__device__ __forceinline__ double cloud_channel(const double *__restrict__ pts, const void *__restrict__ col, int64_t p, int ch)
{
    if (ch < 3) return pts[3 * p + ch];
    if (kCol == kCloudU8) return static_cast<double>(static_cast<const unsigned char *>(col)[3 * p + ch - 3]) / 255.0;
    if (kCol == kCloudF64) return static_cast<const double *>(col)[3 * p + ch - 3];
    return 0.0;
}

// A thread per voxel: a voxel of up to kCloudThreadMax points is put in order where its list lies (insertion
// sort) and folded; a larger one is handed to the block kernels (its number appended to cls_list[0] up to
// kCloudLdsMax points, to cls_list[1] above; cls_n counts them; the order there decides nothing).
template <int kCol>
__global__ __launch_bounds__(256) void k_cloud_fold_small(int nv, const int *__restrict__ voff, int *__restrict__ list,
                                                          const double *__restrict__ pts, const void *__restrict__ col,
                                                          double *__restrict__ out_pts, double *__restrict__ out_col,
                                                          int *__restrict__ cls_n, int *__restrict__ cls_mid,
                                                          int *__restrict__ cls_big)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const int b = voff[v], c = voff[v + 1] - b;
    if (c > kCloudThreadMax) {
        if (c <= kCloudLdsMax) cls_mid[atomicAdd(&cls_n[0], 1)] = v;
        else cls_big[atomicAdd(&cls_n[1], 1)] = v;
        return;
    }
    int *l = list + b;
    for (int a = 1; a < c; a++) {
        const int x = l[a];
        int k = a;
        while (k > 0 && l[k - 1] > x) {
            l[k] = l[k - 1];
            k--;
        }
        l[k] = x;
    }
    constexpr int NC = kCol == kCloudNone ? 3 : 6;
    double s[NC];
#pragma unroll
    for (int ch = 0; ch < NC; ch++) s[ch] = 0.0;
    for (int a = 0; a < c; a++) {
        const int p = l[a];
#pragma unroll
        for (int ch = 0; ch < NC; ch++) s[ch] = s[ch] + cloud_channel<kCol>(pts, col, p, ch);
    }
    const double dc = static_cast<double>(c);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) out_pts[3 * static_cast<int64_t>(v) + ch] = s[ch] / dc;
    if (kCol != kCloudNone)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) out_col[3 * static_cast<int64_t>(v) + ch] = s[3 + ch] / dc;
}

// A workgroup per listed voxel.  kLds: the list (at most kCloudLdsMax entries) is sorted in LDS; otherwise where
// it lies in global memory, the steps of the network separated by sync_global.  The network is
// cloud_sort_partner's.  Then turns of kCloudFoldChunk points: a thread fetches the channels of one point into
// LDS, and threads 0..5 add one channel each, in list order.
template <bool kLds, int kCol, int NT>
__global__ __launch_bounds__(NT) void k_cloud_fold_block(const int *__restrict__ cls_list, const int *__restrict__ voff,
                                                         int *__restrict__ list, const double *__restrict__ pts,
                                                         const void *__restrict__ col, double *__restrict__ out_pts,
                                                         double *__restrict__ out_col)
{
    __shared__ int lds_list[kLds ? kCloudLdsMax : 1];
    __shared__ double stage[6][kCloudFoldChunk];
    const int v = cls_list[blockIdx.x];
    const int b = voff[v], c = voff[v + 1] - b;
    if (kLds && c > kCloudLdsMax) return;  // (not listed here: k_cloud_fold_small sorts the voxels by population)
    int *arr = kLds ? lds_list : list + b;
    if (kLds) {
        for (int i = threadIdx.x; i < c; i += NT) lds_list[i] = list[b + i];
        __syncthreads();
    }
    for (int64_t k = 2; (k >> 1) < c; k <<= 1)
        for (int64_t j = 0, next = k >> 2;; j = next, next >>= 1) {  // j = 0 (the mirror step), k/4, k/8, ... 1
            for (int i = threadIdx.x; i < c; i += NT) {
                const int64_t l = cloud_sort_partner(i, k, j, c);
                if (l < 0) continue;
                const int x = arr[i], y = arr[l];
                if (x > y) arr[i] = y, arr[l] = x;
            }
            if (kLds) __syncthreads();
            else sync_global();
            if (next < 1) break;
        }
    constexpr int NC = kCol == kCloudNone ? 3 : 6;
    double s = 0.0;
    for (int base = 0; base < c; base += kCloudFoldChunk) {
        const int m = min(kCloudFoldChunk, c - base);
        if (threadIdx.x < m) {
            const int p = arr[base + threadIdx.x];
#pragma unroll
            for (int ch = 0; ch < NC; ch++) stage[ch][threadIdx.x] = cloud_channel<kCol>(pts, col, p, ch);
        }
        __syncthreads();
        if (threadIdx.x < NC)
            for (int a = 0; a < m; a++) s = s + stage[threadIdx.x][a];
        __syncthreads();
    }
    if (threadIdx.x < NC) {
        const double q = s / static_cast<double>(c);
        if (threadIdx.x < 3) out_pts[3 * static_cast<int64_t>(v) + threadIdx.x] = q;
        else out_col[3 * static_cast<int64_t>(v) + threadIdx.x - 3] = q;
    }
}

// the result's points rounded to float32 (round to nearest even: torch.tensor(...).float())
__global__ __launch_bounds__(256) void k_cloud_to_f32(int64_t n, const double *__restrict__ in, float *__restrict__ out)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) out[i] = static_cast<float>(in[i]);
}

}  // namespace mc
