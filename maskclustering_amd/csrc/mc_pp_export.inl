// mc_pp_export.inl — the export of the final objects (utils/post_process.py:126-128, 148-165): pp_build_export
// and mc_pp_export_pred_masks of mc_pp_host.inl.  Included by mc_pp_kernels.inl.

namespace mc {

// Entries of [a, b) whose key is o, in order, by one 256-thread workgroup: each wave counts its
// contiguous quarter, then compacts it behind the waves before it.  emit(entry, position).
template <typename Emit>
__device__ __forceinline__ void pp_compact256(int64_t a, int64_t b, const int *__restrict__ key, int o, int *ws,
                                              Emit &&emit)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t per = (((b - a) + 3) / 4 + 63) / 64 * 64;
    const int64_t s0 = min(b, a + wv * per), s1 = min(b, s0 + per);
    int cnt = 0;
    for (int64_t i = s0 + lane; i < s1; i += 64) cnt += key[i] == o;
    cnt = wave_sum(cnt);
    if (lane == 0) ws[wv] = cnt;
    __syncthreads();
    int64_t base = 0;
    for (int w = 0; w < wv; w++) base += ws[w];
    for (int64_t i0 = s0; i0 < s1; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool hit = i < s1 && key[i] == o;
        const unsigned long long m = __ballot(hit);
        if (hit) emit(i, base + __popcll(m & ((1ull << lane) - 1)));
        base += __popcll(m);
    }
    __syncthreads();
}

// per final object (a workgroup each): its kept points in its node's point order, the masks
// assigned to it in the node's mask_list order with their coverages
__global__ __launch_bounds__(256) void k_pp_ex_fill(int nfin, const int *__restrict__ fin_obj,
                                                    const int *__restrict__ fin_node, const int64_t *__restrict__ npoff,
                                                    const int *__restrict__ npts, const int *__restrict__ ent_obj,
                                                    const int64_t *__restrict__ qoff, const int *__restrict__ qm,
                                                    const int *__restrict__ qobj, const double *__restrict__ qcov,
                                                    const int64_t *__restrict__ opoff, int *__restrict__ opts,
                                                    const int64_t *__restrict__ omoff, int *__restrict__ omask,
                                                    double *__restrict__ ocov)
{
    __shared__ int ws[4];
    for (int f = blockIdx.x; f < nfin; f += gridDim.x) {
        const int o = fin_obj[f], k = fin_node[f];
        const int64_t pb = opoff[f], pe = opoff[f + 1], mb = omoff[f], me = omoff[f + 1];
        pp_compact256(npoff[k], npoff[k + 1], ent_obj, o, ws, [&](int64_t e, int64_t pos) {
            if (pb + pos < pe) opts[pb + pos] = npts[e];
        });
        pp_compact256(qoff[k], qoff[k + 1], qobj, o, ws, [&](int64_t q, int64_t pos) {
            if (mb + pos < me) {
                omask[mb + pos] = qm[q];
                ocov[mb + pos] = qcov[q];
            }
        });
    }
}

// The order of find_represent_mask's sort (:126-128), by one wave: the positions of the k largest of
// the n coverages cov[0 .. n), equal coverages in list order (Python's sort is stable), INT_MAX
// past the end.  emit(rank, position) runs in every lane with the same arguments.
template <typename Emit>
__device__ __forceinline__ void pp_cov_top(const double *__restrict__ cov, int n, int k, int lane, Emit &&emit)
{
    double pc = 0.0;  // the pick before this one
    int pp = -1;
    for (int r = 0; r < k; r++) {
        double bc = 0.0;
        int bp = INT_MAX;
        for (int i = lane; i < n; i += 64) {
            const double c = cov[i];
            const bool after = pp < 0 || c < pc || (c == pc && i > pp);
            if (after && (bp == INT_MAX || c > bc)) {
                bc = c;
                bp = i;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double oc = __shfl_xor(bc, d, 64);
            const int op = __shfl_xor(bp, d, 64);
            if (op != INT_MAX && (bp == INT_MAX || oc > bc || (oc == bc && op < bp))) {
                bc = oc;
                bp = op;
            }
        }
        emit(r, bp);
        if (bp == INT_MAX) {  // (uniform) nothing left
            pp = n;
            pc = -1.0;
        } else {
            pc = bc;
            pp = bp;
        }
    }
}

// find_represent_mask (:126-128): positions of the five largest coverages in an object's mask list,
// -1 past the end; a wave per object
__global__ __launch_bounds__(256) void k_pp_ex_repre(int nfin, const int64_t *__restrict__ omoff,
                                                     const double *__restrict__ ocov, int *__restrict__ repre)
{
    const int lane = lane_id();
    for (int f = blockIdx.x * 4 + (threadIdx.x >> 6); f < nfin; f += gridDim.x * 4) {
        const int64_t a = omoff[f];
        const int n = static_cast<int>(omoff[f + 1] - a);
        pp_cov_top(ocov + a, n, 5, lane, [&](int r, int bp) {
            if (lane == 0) repre[5 * f + r] = bp == INT_MAX ? -1 : bp;
        });
    }
}

// the [P, nfin] uint8 matrix of the prediction file (:148-165): 1 where the object keeps the point
__global__ __launch_bounds__(256) void k_pp_ex_pred(int64_t E, const int *__restrict__ npts, const int *__restrict__ ent_obj,
                                                    const int *__restrict__ fslot, int nfin, unsigned char *__restrict__ out)
{
    for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < E; e += gridDim.x * 256ll) {
        const int o = ent_obj[e];
        if (o < 0) continue;
        const int s = fslot[o];
        if (s >= 0) out[static_cast<int64_t>(npts[e]) * nfin + s] = 1;
    }
}

}  // namespace mc
