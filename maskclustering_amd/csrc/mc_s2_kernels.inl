// mc_s2_kernels.inl — S2 point-in-mask structure (graph/construction.py:22-64); included by mc_kernels.inl.
// Launched by graph_s2_point_lists (mc_graph_host.inl); k_s2_dense_pim by the getter mc_graph_get_point_in_mask.
namespace mc {

// deg[p] += 1 for every (mask, point) entry.  Block 0 also clears the statistics block.
__global__ __launch_bounds__(256) void k_s2_degree(const int *__restrict__ pts, int nnz, int *__restrict__ deg,
                                                   int *__restrict__ stats, int nstats, int *__restrict__ spread)
{
    if (blockIdx.x == 0 && threadIdx.x < nstats) stats[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x < kSpread) spread[threadIdx.x * kSpreadStrideI] = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nnz; i += gridDim.x * 256) atomicAdd(&deg[pts[i]], 1);
}

// One workgroup per mask: append (frame << 12 | mask-in-frame) to each point's list.
// deg[] counts down to zero again (ready for the next build, no memset).
__global__ __launch_bounds__(256) void k_s2_scatter(const int *__restrict__ mask_off, const int *__restrict__ pts,
                                                    const int *__restrict__ mask_col,
                                                    const int *__restrict__ frame_start,
                                                    const int *__restrict__ pt_off, int *__restrict__ deg,
                                                    unsigned *__restrict__ pt_list)
{
    const int g = blockIdx.x;
    const int c = mask_col[g];
    const unsigned e = (static_cast<unsigned>(c) << kLocalBits) | static_cast<unsigned>(g - frame_start[c]);
    const int b = mask_off[g], en = mask_off[g + 1];
    for (int k = b + threadIdx.x; k < en; k += 256) {
        const int p = pts[k];
        const int pos = pt_off[p] + atomicSub(&deg[p], 1) - 1;
        pt_list[pos] = e;
    }
}

// Sort one point's list (in LDS or global), flag the point as boundary if one frame
// appears twice (>= 2 masks in one frame: construction.py:56,61-62) and write its
// point-frame bits (construction.py:52).
__device__ __forceinline__ int s2_point_row(unsigned *lst, int n, int FW, unsigned long long *pfm_row)
{
    for (int i = 1; i < n; i++) {
        const unsigned x = lst[i];
        int j = i - 1;
        while (j >= 0 && lst[j] > x) {
            lst[j + 1] = lst[j];
            j--;
        }
        lst[j + 1] = x;
    }
    int isb = 0;
    unsigned prevc = 0xffffffffu;
    int q = 0;
    for (int w = 0; w < FW; w++) {
        unsigned long long word = 0;
        while (q < n) {
            const unsigned c = lst[q] >> kLocalBits;
            if (static_cast<int>(c >> 6) != w) break;
            if (c == prevc) isb = 1;
            prevc = c;
            word |= 1ull << (c & 63);
            q++;
        }
        pfm_row[w] = word;
    }
    return isb;
}

// 256 consecutive points per workgroup; their lists are one contiguous range of pt_list,
// staged through LDS when it fits (coalesced load, LDS sort, coalesced store).
constexpr int kS2Stage = 8192;

__global__ __launch_bounds__(256) void k_s2_points(const int *__restrict__ pt_off, unsigned *__restrict__ pt_list,
                                                   int P, int FW, unsigned char *__restrict__ boundary,
                                                   unsigned long long *__restrict__ pfm, int *__restrict__ nbnd)
{
    __shared__ unsigned stage[kS2Stage];
    const int p0 = blockIdx.x * 256;
    const int p = p0 + threadIdx.x;
    const int pend = min(P, p0 + 256);
    const int eb = pt_off[p0], ee = pt_off[pend];
    const bool staged = (ee - eb) <= kS2Stage;
    int isb = 0;
    if (staged) {
        for (int i = threadIdx.x; i < ee - eb; i += 256) stage[i] = pt_list[eb + i];
        __syncthreads();
        if (p < P) {
            const int b = pt_off[p] - eb, e = pt_off[p + 1] - eb;
            isb = s2_point_row(stage + b, e - b, FW, pfm + static_cast<size_t>(p) * FW);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < ee - eb; i += 256) pt_list[eb + i] = stage[i];
    } else if (p < P) {
        const int b = pt_off[p], e = pt_off[p + 1];
        isb = s2_point_row(pt_list + b, e - b, FW, pfm + static_cast<size_t>(p) * FW);
    }
    if (p < P) boundary[p] = static_cast<unsigned char>(isb);
    const unsigned long long bal = __ballot(isb);
    if (lane_id() == 0 && bal) spread_add(nbnd, __popcll(bal));  // folded by k_s3_undo_count
}

// Dense point_in_mask_matrix (uint16 P×F) for the getter only (construction.py:39,58,61).
__global__ __launch_bounds__(256) void k_s2_dense_pim(const int *__restrict__ pt_off, const unsigned *__restrict__ pt_list,
                                                      const int *__restrict__ mask_label,
                                                      const int *__restrict__ frame_start, int P, int F,
                                                      unsigned short *__restrict__ pim)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int b = pt_off[p], e = pt_off[p + 1];
    unsigned short *row = pim + static_cast<size_t>(p) * F;
    for (int i = b; i < e; i++) {
        unsigned c = pt_list[i] >> kLocalBits;
        bool dup = (i > b && (pt_list[i - 1] >> kLocalBits) == c) || (i + 1 < e && (pt_list[i + 1] >> kLocalBits) == c);
        if (!dup) row[c] = static_cast<unsigned short>(mask_label[frame_start[c] + (pt_list[i] & (kMaxMasksPerFrame - 1))]);
    }
}

}  // namespace mc
