// mc_pp_layout.inl — the checks of the argument arrays and the per-node layout of all three entries (pp_layout,
// mc_pp_host.inl), and the node arrays of the clustered objects (mc_pp_run_clustered).  Included by
// mc_pp_kernels.inl.

namespace mc {

// the argument arrays of mc_pp_run, as device pointers
struct PPArgs {
    int64_t P, E, Q, MP;
    int F, FW, Mt, N;
    const double *scene;
    const unsigned long long *pfm, *nvf;
    const int64_t *mask_off, *npoff, *qoff;
    const int *mask_pts, *npts, *qm, *qcol;
};

// bits of the check flag
constexpr int kPPBadOffsets = 1;  // offsets not ascending
constexpr int kPPBadIndex = 2;    // a point / mask / frame index out of range
constexpr int kPPBadFrame = 4;    // a mask's frame is not visible to its node (post_process.py:69)
constexpr int kPPTooWide = 8;     // a node spans more than 2^21 DBSCAN cells

// Range checks of the argument arrays.  Reads the arrays at positions below their host-known sizes
// only, never at a position taken from their contents; every later kernel runs behind this flag.
__global__ __launch_bounds__(256) void k_pp_validate(PPArgs a, int *__restrict__ flag)
{
    const int64_t tot = max(max(a.E, a.MP), max(a.Q, static_cast<int64_t>(max(a.N, a.Mt))));
    int bad = 0;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < tot; i += gridDim.x * 256ll) {
        if (i < a.N && (a.npoff[i] < 0 || a.npoff[i + 1] < a.npoff[i] || a.npoff[i + 1] > a.E || a.qoff[i] < 0 ||
                        a.qoff[i + 1] < a.qoff[i] || a.qoff[i + 1] > a.Q))
            bad |= kPPBadOffsets;
        if (i < a.Mt && (a.mask_off[i] < 0 || a.mask_off[i + 1] < a.mask_off[i] || a.mask_off[i + 1] > a.MP))
            bad |= kPPBadOffsets;
        if (i < a.E && (a.npts[i] < 0 || a.npts[i] >= a.P)) bad |= kPPBadIndex;
        if (i < a.MP && (a.mask_pts[i] < 0 || a.mask_pts[i] >= a.P)) bad |= kPPBadIndex;
        if (i < a.Q && (a.qm[i] < 0 || a.qm[i] >= a.Mt || a.qcol[i] < 0 || a.qcol[i] >= a.F)) bad |= kPPBadIndex;
    }
    if (bad) atomicOr(flag, bad);
}

// Per node (a workgroup each): the number of visible frames, each mask's rank among them (qfpos,
// post_process.py:67-69), the hit-bit words of the node (points x ceil(visible / 64)), its size, and
// its extent against the 2^21 cells per axis the DBSCAN grid packs.  Does nothing when k_pp_validate
// found a bad offset or index.
__global__ __launch_bounds__(256) void k_pp_prep(PPArgs a, PPDev pr, int *__restrict__ flag, int *__restrict__ qfpos,
                                                 int64_t *__restrict__ hit_words, int *__restrict__ nsize)
{
    __shared__ double red[6 * 4];
    __shared__ int ws[4];
    if (ld_agent(flag) & (kPPBadOffsets | kPPBadIndex)) return;  // set by the kernel before only: uniform
    const int t = threadIdx.x;
    for (int k = blockIdx.x; k < a.N; k += gridDim.x) {
        const unsigned long long *vf = a.nvf + static_cast<int64_t>(k) * a.FW;
        int c = 0;
        for (int w = t; w < a.FW; w += 256) c += __popcll(vf[w]);
        const int nvis = block_sum<256>(c, ws);
        for (int64_t q = a.qoff[k] + t; q < a.qoff[k + 1]; q += 256) {
            const int col = a.qcol[q];
            int pos = 0;
            if ((vf[col >> 6] >> (col & 63)) & 1ull) {
                for (int w = 0; w < (col >> 6); w++) pos += __popcll(vf[w]);
                pos += __popcll(vf[col >> 6] & ((1ull << (col & 63)) - 1));
            } else
                atomicOr(flag, kPPBadFrame);
            qfpos[q] = pos;
        }
        const int64_t e0 = a.npoff[k], e1 = a.npoff[k + 1];
        double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, mx[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
        for (int64_t i = e0 + t; i < e1; i += 256) {
            const double *p = a.scene + 3 * static_cast<int64_t>(a.npts[i]);
#pragma unroll
            for (int d = 0; d < 3; d++) {
                mn[d] = fmin(mn[d], p[d]);
                mx[d] = fmax(mx[d], p[d]);
            }
        }
        pp_block_minmax3<256>(mn, mx, red);
        if (t == 0) {
            for (int d = 0; d < 3; d++)
                if (mx[d] >= mn[d] && !(floor((mx[d] - mn[d]) / pr.ce) < kPPMaxCells))
                    atomicOr(flag, kPPTooWide);
            hit_words[k] = (e1 - e0) * ((nvis + 63) / 64);
            nsize[k] = static_cast<int>(e1 - e0);
        }
    }
}

// the size order: nodes by descending point count, equal sizes in node order (a rank per node)
__global__ __launch_bounds__(256) void k_pp_order(int N, const int *__restrict__ nsize, const int *__restrict__ flag,
                                                  int *__restrict__ order)
{
    if (ld_agent(flag) & (kPPBadOffsets | kPPBadIndex)) return;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < N; k += gridDim.x * 256) {
        const int s = nsize[k];
        int r = 0;
        for (int j = 0; j < N; j++) {
            const int sj = nsize[j];
            r += sj > s || (sj == s && j < k);
        }
        order[r] = k;
    }
}

// exclusive scan of n values into n + 1 int64 offsets by one 1024-thread workgroup (n = nodes or
// masks: each thread sums a contiguous run, the run sums are scanned in LDS).  in != out.
template <typename T>
__global__ __launch_bounds__(1024) void k_pp_scan64(const T *__restrict__ in, int n, int64_t *__restrict__ out)
{
    __shared__ int64_t part[1024];
    const int t = threadIdx.x, per = (n + 1023) / 1024;
    const int a = min(n, t * per), b = min(n, a + per);
    int64_t s = 0;
    for (int i = a; i < b; i++) s += in[i];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t ex = part[t] - s;
    for (int i = a; i < b; i++) {
        out[i] = ex;
        ex += in[i];
    }
    if (t == 1023) out[n] = part[1023];
}

__global__ __launch_bounds__(256) void k_pp_widen(const float *__restrict__ in, int64_t n, double *__restrict__ out)
{
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) out[i] = static_cast<double>(in[i]);
}

// ---- node arrays of the clustered objects (mc_pp_run_clustered) ----
__global__ __launch_bounds__(256) void k_pp_cl_count(int N0, const int *__restrict__ label, int *__restrict__ cnt)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N0; i += gridDim.x * 256) atomicAdd(&cnt[label[i]], 1);
}

__global__ __launch_bounds__(256) void k_pp_cl_keep(int K, const int *__restrict__ cnt, int *__restrict__ keep)
{
    for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) keep[k] = cnt[k] >= 2;  // post_process.py:182
}

// the kept objects in object-id order: their object, point count and mask count
__global__ __launch_bounds__(256) void k_pp_cl_select(int K, const int *__restrict__ cnt, const int *__restrict__ nid,
                                                      const int *__restrict__ obj_ptoff, int *__restrict__ sel,
                                                      int *__restrict__ plen, int *__restrict__ mlen)
{
    for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) {
        if (cnt[k] < 2) continue;
        const int j = nid[k];
        sel[j] = k;
        plen[j] = obj_ptoff[k + 1] - obj_ptoff[k];
        mlen[j] = cnt[k];
    }
}

// point count of every row of the mask table in input order (rows of skipped frames hold none)
__global__ __launch_bounds__(256) void k_pp_cl_masklen(int M, const int *__restrict__ in_index,
                                                       const int *__restrict__ mask_off, int *__restrict__ len)
{
    for (int g = blockIdx.x * 256 + threadIdx.x; g < M; g += gridDim.x * 256)
        len[in_index ? in_index[g] : g] = mask_off[g + 1] - mask_off[g];
}

// A node's masks: its level-0 members in ascending level-0 node id, a wave per node walking the
// labels in order (a stable grouping without atomics); each as its row of the mask table in input
// order, with its frame column.
__global__ __launch_bounds__(256) void k_pp_cl_members(int Nn, int N0, const int *__restrict__ sel,
                                                       const int *__restrict__ label, const int *__restrict__ node0_g,
                                                       const int *__restrict__ in_index, const int *__restrict__ mask_col,
                                                       const int64_t *__restrict__ qoff, int *__restrict__ qm,
                                                       int *__restrict__ qcol)
{
    const int lane = lane_id();
    for (int j = blockIdx.x * 4 + (threadIdx.x >> 6); j < Nn; j += gridDim.x * 4) {
        const int k = sel[j];
        int64_t pos = qoff[j];
        for (int i0 = 0; i0 < N0; i0 += 64) {
            const int i = i0 + lane;
            const bool hit = i < N0 && label[i] == k;
            const unsigned long long m = __ballot(hit);
            if (hit) {
                const int64_t q = pos + __popcll(m & ((1ull << lane) - 1));
                const int g = node0_g[i];
                qm[q] = in_index ? in_index[g] : g;
                qcol[q] = mask_col[g];
            }
            pos += __popcll(m);
        }
    }
}

// a node's points (the object's, in the order mc_cluster_get_objects returns them) and visible frames
__global__ __launch_bounds__(256) void k_pp_cl_gather(int Nn, int FW, const int *__restrict__ sel,
                                                      const int *__restrict__ obj_ptoff, const int *__restrict__ obj_pts,
                                                      const unsigned long long *__restrict__ obj_vf,
                                                      const int64_t *__restrict__ npoff, int *__restrict__ npts,
                                                      unsigned long long *__restrict__ nvf)
{
    for (int j = blockIdx.x; j < Nn; j += gridDim.x) {
        const int k = sel[j];
        const int a = obj_ptoff[k], n = obj_ptoff[k + 1] - a;
        const int64_t e0 = npoff[j];
        for (int i = threadIdx.x; i < n; i += 256) npts[e0 + i] = obj_pts[a + i];
        for (int w = threadIdx.x; w < FW; w += 256)
            nvf[static_cast<int64_t>(j) * FW + w] = obj_vf[static_cast<int64_t>(k) * FW + w];
    }
}

}  // namespace mc
