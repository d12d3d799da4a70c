// mc_pp_filter.inl — filter_point (utils/post_process.py:40-101): pp_filter of mc_pp_host.inl launches
// k_pp_filter.  Included by mc_pp_kernels.inl.

namespace mc {

// wave-wide first maximum (value, index): larger value wins, smaller index on ties
__device__ __forceinline__ void pp_wave_argmax(int &v, int &ix)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int ov = __shfl_xor(v, d, 64), oi = __shfl_xor(ix, d, 64);
        if (ov > v || (ov == v && oi < ix)) {
            v = ov;
            ix = oi;
        }
    }
}

// filter_point (post_process.py:40-101) of every node; posmap = one P-entry map per workgroup,
// -1 at rest.
__global__ __launch_bounds__(256) void k_pp_filter(
    int N, const int *__restrict__ order, int *__restrict__ ticket, PPDev pr, int FW, int64_t P,
    const int64_t *__restrict__ pt_off, const int *__restrict__ pts, const unsigned long long *__restrict__ nvf,
    const int64_t *__restrict__ hit_off, const int64_t *__restrict__ qoff, const int *__restrict__ qmask,
    const int *__restrict__ qfpos, const int64_t *__restrict__ mask_off, const int *__restrict__ mask_pts,
    const unsigned long long *__restrict__ pfm, const double *__restrict__ xyz, const int *__restrict__ lab,
    const int *__restrict__ ccnt, const int *__restrict__ nob, const int *__restrict__ nsh,
    const int *__restrict__ obj_base,
    int *__restrict__ posmap, unsigned long long *__restrict__ hit, int *__restrict__ cvid,
    int *__restrict__ qobj, double *__restrict__ qcov, int *__restrict__ obj_nmask, int *__restrict__ obj_nvalid,
    double *__restrict__ obj_box, int *__restrict__ ent_obj)
{
    __shared__ int s_cnt[4][kPPObjChunk];
    __shared__ unsigned long long s_box[kPPBoxChunk * 6];
    __shared__ int s_nv[kPPBoxChunk];
    __shared__ int s_k;
    const int t = threadIdx.x, lane = lane_id(), wv = t >> 6;
    int *pm = posmap + static_cast<int64_t>(blockIdx.x) * P;
    while (true) {
        if (t == 0) s_k = atomicAdd(ticket, 1);
        sync_global();
        const int kk = s_k;
        sync_global();
        if (kk >= N) break;
        const int k = order[kk];
        const int64_t e0 = pt_off[k];
        const int n = static_cast<int>(pt_off[k + 1] - e0);
        const int no = nob[k], sh = nsh[k], ob = obj_base[k];
        const int *lb = lab + e0, *cc = ccnt + e0 + k;
        const int W = n ? static_cast<int>((hit_off[k + 1] - hit_off[k]) / n) : 0;
        unsigned long long *hk = hit + hit_off[k];
        const unsigned long long *vf = nvf + static_cast<int64_t>(k) * FW;
        // 1. position map; frames of the node's visible frames the point is seen in (:45-58)
        for (int i = t; i < n; i += 256) {
            const int p = pts[e0 + i];
            pm[p] = i;
            int c = 0;
            for (int w = 0; w < FW; w++) c += __popcll(pfm[static_cast<int64_t>(p) * FW + w] & vf[w]);
            cvid[e0 + i] = c;
        }
        sync_global();
        // 2. masks of the node, a wave each (:68-81): frame bits of the points they hold, and the
        //    object of largest intersection
        const int64_t q0 = qoff[k], q1 = qoff[k + 1];
        for (int64_t q = q0 + wv; q < q1; q += 4) {
            const int m = qmask[q], fp = qfpos[q];
            const int64_t a = mask_off[m], b = mask_off[m + 1];
            int best = -1, largest = 0;
            for (int c0 = 0; c0 < no; c0 += kPPObjChunk) {
                const int cn = min(kPPObjChunk, no - c0);
                for (int c = lane; c < cn; c += 64) s_cnt[wv][c] = 0;
                __builtin_amdgcn_wave_barrier();
                for (int64_t j = a + lane; j < b; j += 64) {
                    const int li = pm[mask_pts[j]];
                    if (li < 0) continue;
                    if (c0 == 0) atomicOr(&hk[static_cast<int64_t>(li) * W + (fp >> 6)], 1ull << (fp & 63));
                    const int o = lb[li] - sh - c0;
                    if (o >= 0 && o < cn) atomicAdd(&s_cnt[wv][o], 1);
                }
                __builtin_amdgcn_wave_barrier();
                int v = 0, ix = INT_MAX;
                for (int c = lane; c < cn; c += 64) {
                    const int x = s_cnt[wv][c];
                    if (x > v) {
                        v = x;
                        ix = c;
                    }
                }
                pp_wave_argmax(v, ix);
                if (v > largest) {
                    largest = v;
                    best = c0 + ix;
                }
                __builtin_amdgcn_wave_barrier();
            }
            if (lane == 0) {
                qobj[q] = best >= 0 ? ob + best : -1;
                qcov[q] = best >= 0 ? static_cast<double>(largest) / static_cast<double>(cc[best + sh]) : 0.0;
                if (best >= 0) atomicAdd(&obj_nmask[ob + best], 1);
            }
        }
        sync_global();
        // 3. detection ratio (:93-95), kept-point counts and bboxes of all object points (:99)
        for (int c0 = 0; c0 < no; c0 += kPPBoxChunk) {
            const int cn = min(kPPBoxChunk, no - c0);
            for (int c = t; c < cn; c += 256) {
                s_nv[c] = 0;
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    s_box[6 * c + d] = ~0ull;
                    s_box[6 * c + 3 + d] = 0ull;
                }
            }
            sync_global();
            for (int i = t; i < n; i += 256) {
                const int o = lb[i] - sh;
                int cnode = 0;
                for (int w = 0; w < W; w++)
                    cnode += __popcll(__hip_atomic_load(&hk[static_cast<int64_t>(i) * W + w], __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT));
                const bool valid = static_cast<double>(cnode) / (static_cast<double>(cvid[e0 + i]) + 1e-6) > pr.thr;
                if (c0 == 0) ent_obj[e0 + i] = valid ? ob + o : -1;
                if (o - c0 < 0 || o - c0 >= cn) continue;
                const int oc = o - c0;
                if (valid) atomicAdd(&s_nv[oc], 1);
#pragma unroll
                for (int d = 0; d < 3; d++) {
                    const unsigned long long u = pp_ord(xyz[3 * (e0 + i) + d]);
                    atomicMin(&s_box[6 * oc + d], u);
                    atomicMax(&s_box[6 * oc + 3 + d], u);
                }
            }
            sync_global();
            for (int c = t; c < cn; c += 256) {
                obj_nvalid[ob + c0 + c] = s_nv[c];
#pragma unroll
                for (int d = 0; d < 6; d++) obj_box[6 * static_cast<int64_t>(ob + c0 + c) + d] = pp_unord(s_box[6 * c + d]);
            }
            sync_global();
        }
        // 4. the position map returns to -1
        for (int i = t; i < n; i += 256) pm[pts[e0 + i]] = -1;
        sync_global();
    }
}

}  // namespace mc
