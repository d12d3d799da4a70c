// mc_pp_merge.inl — merge_overlapping_objects (utils/post_process.py:7-37): pp_merge of mc_pp_host.inl
// launches these in order.  Included by mc_pp_kernels.inl.

namespace mc {

// intersection index: the kept objects holding each point (fixed slots; overflow -> regrow)
__global__ __launch_bounds__(256) void k_pp_index(int64_t E, const int *__restrict__ pts, const int *__restrict__ ent_obj,
                                                  const int *__restrict__ kidx, int slots, int *__restrict__ pcnt,
                                                  int *__restrict__ plist, int *__restrict__ maxcnt)
{
    for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < E; e += gridDim.x * 256ll) {
        const int o = ent_obj[e];
        if (o < 0) continue;
        const int kk = kidx[o];
        if (kk < 0) continue;
        const int p = pts[e];
        const int s = atomicAdd(&pcnt[p], 1);
        if (s < slots) plist[static_cast<int64_t>(p) * slots + s] = kk;
        atomicMax(maxcnt, s + 1);
    }
}

// |set_i ∩ set_j| for every pair of kept objects sharing a point (dense K x K, i < j)
__global__ __launch_bounds__(256) void k_pp_pairs(int64_t P, int slots, const int *__restrict__ pcnt,
                                                  const int *__restrict__ plist, int K, int *__restrict__ inter)
{
    for (int64_t p = blockIdx.x * 256ll + threadIdx.x; p < P; p += gridDim.x * 256ll) {
        const int c = pcnt[p];
        if (c < 2) continue;
        const int *l = plist + p * slots;
        for (int a = 0; a < c; a++)
            for (int b = a + 1; b < c; b++) {
                const int x = min(l[a], l[b]), y = max(l[a], l[b]);
                atomicAdd(&inter[static_cast<int64_t>(x) * K + y], 1);
            }
    }
}

// decision of every pair i < j (post_process.py:24-29): 1 = i merged away, 2 = j merged away
// The non-zero decisions are also appended to a list (order-free; capacity cap) so that the host
// can run the greedy pass over them alone when they fit.
__global__ __launch_bounds__(256) void k_pp_decide(int K, PPDev pr, const double *__restrict__ box,
                                                   const int *__restrict__ len, const int *__restrict__ inter,
                                                   unsigned char *__restrict__ dec, int cap, int *__restrict__ nlist,
                                                   int2 *__restrict__ list)
{
    const int64_t tot = static_cast<int64_t>(K) * K;
    for (int64_t x = blockIdx.x * 256ll + threadIdx.x; x < tot; x += gridDim.x * 256ll) {
        const int i = static_cast<int>(x / K), j = static_cast<int>(x % K);
        if (j <= i) continue;
        const double *bi = box + 6 * static_cast<int64_t>(i), *bj = box + 6 * static_cast<int64_t>(j);
        bool ov = true;
#pragma unroll
        for (int d = 0; d < 3; d++)
            if (bi[d] > bj[3 + d] || bj[d] > bi[3 + d]) ov = false;  // utils/geometry.py:3-7
        unsigned char r = 0;
        if (ov) {
            const double in = static_cast<double>(inter[x]);
            if (in / static_cast<double>(len[i]) > pr.ratio) r = 1;
            else if (in / static_cast<double>(len[j]) > pr.ratio) r = 2;
        }
        dec[x] = r;
        if (r) {
            const int at = atomicAdd(nlist, 1);
            if (at < cap) list[at] = make_int2(i, r == 1 ? -1 - j : j);
        }
    }
}

// the greedy pass (post_process.py:14-29): sequential in i, every j of one i in parallel
__global__ __launch_bounds__(1024) void k_pp_greedy(int K, const unsigned char *__restrict__ dec,
                                                    unsigned char *__restrict__ inv)
{
    __shared__ int s_flag;
    const int t = threadIdx.x;
    for (int i = t; i < K; i += 1024) inv[i] = 0;
    sync_global();
    for (int i = 0; i < K; i++) {
        if (t == 0) s_flag = 0;
        sync_global();
        if (inv[i]) continue;  // uniform: written before the last barrier
        const unsigned char *d = dec + static_cast<int64_t>(i) * K;
        int f = 0;
        for (int j = i + 1 + t; j < K; j += 1024) {
            if (inv[j]) continue;
            const unsigned char r = d[j];
            if (r == 1) f = 1;
            else if (r == 2) inv[j] = 1;
        }
        if (f) s_flag = 1;
        sync_global();
        if (t == 0 && s_flag) inv[i] = 1;
        sync_global();
    }
}

}  // namespace mc
