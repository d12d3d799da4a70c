// mc_bp_batch.inl — S1 back-projection: a batch's bookkeeping around the steps: the status block
// cleared at its start (bp_launch_pixels), its kept masks and statistics written out at its end
// (bp_emit_pack).
namespace mc {

// kept masks -> output CSR (one wave per slot)
__global__ __launch_bounds__(256) void k_bp_emit(const int *__restrict__ dNS, const int *__restrict__ slot_frame,
                                                 const int *__restrict__ slot_id, const int *__restrict__ slot_nn,
                                                 const int *__restrict__ slot_toff, const int *__restrict__ midx,
                                                 const int *__restrict__ moff, const int *__restrict__ tmp,
                                                 int *__restrict__ out_col, int *__restrict__ out_label,
                                                 int *__restrict__ out_off, int *__restrict__ out_pts)
{
    const int NS = *dNS;
    const int lane = lane_id();
    for (int s = (blockIdx.x * 256 + threadIdx.x) >> 6; s < NS; s += gridDim.x * 4) {
        const int nn = slot_nn[s];
        if (nn < 0) continue;
        const int g = midx[s], o = moff[s], src = slot_toff[s];
        if (lane == 0) {
            out_col[g] = slot_frame[s];
            out_label[g] = slot_id[s];
            out_off[g] = o;
        }
        for (int x = lane; x < nn; x += 64) out_pts[o + x] = tmp[src + x];
    }
}

// per-batch statistics block: the error frame at INT_MAX, every counter and ticket zero (a kernel
// instead of a pageable host-to-device copy at every batch start)
// ring-search queue regions: class c's entries start at the voxels of the classes before it
// (per_class 0: one region for every class, at 0)
__global__ __launch_bounds__(64) void k_bp_stat_init(int *__restrict__ st, int n)
{
    for (int i = threadIdx.x; i < n; i += 64) st[i] = i == 0 ? INT_MAX : 0;
}

// Per-batch readback in one copy: [col | label | off] of the batch's Mb kept masks, then the 8
// per-slot statistics arrays of its NS slots, contiguous in `out`
__global__ __launch_bounds__(256) void k_bp_pack(const int *__restrict__ dNS, const int *__restrict__ dM,
                                                 const int *__restrict__ col, const int *__restrict__ lab,
                                                 const int *__restrict__ off, const int *__restrict__ s0,
                                                 const int *__restrict__ s1, const int *__restrict__ s2,
                                                 const int *__restrict__ s3, const int *__restrict__ s4,
                                                 const int *__restrict__ s5, const int *__restrict__ s6,
                                                 const int *__restrict__ s7, int *__restrict__ out)
{
    const int NS = *dNS, M = *dM;
    const int *src[11] = {col, lab, off, s0, s1, s2, s3, s4, s5, s6, s7};
    const size_t total = 3 * static_cast<size_t>(M) + 8 * static_cast<size_t>(NS);
    for (size_t x = blockIdx.x * 256 + threadIdx.x; x < total; x += static_cast<size_t>(gridDim.x) * 256) {
        int a, i;
        if (x < 3 * static_cast<size_t>(M)) {
            a = static_cast<int>(x / M);
            i = static_cast<int>(x % M);
        } else {
            const size_t y = x - 3 * static_cast<size_t>(M);
            a = 3 + static_cast<int>(y / NS);
            i = static_cast<int>(y % NS);
        }
        out[x] = src[a][i];
    }
}

}  // namespace mc
