// mc_proj_kernels.inl — device code of the projected boxes (mc_proj_*; get_top_images.py:180-237).
// The per-point arithmetic, the accumulator and the status rule are mc_proj_plan.hpp's.
//   k_proj_validate    range checks of mc_proj_boxes' device arrays behind one flag word, and the
//                      largest requested object
//   k_proj_init        every request's accumulator at rest
//   k_proj_accum       workgroup per (request group, part): the object's points gathered once and
//                      projected into each of the group's up to kProjMaxTop frames
//   k_proj_finish      accumulator -> box, status, in-bounds count (-1 for a padded request)
//   k_proj_ocol        per final object of the last post-processing run: its masks' frame columns
//   k_proj_top_select  per final object: the first top_k mask-list positions by coverage (the
//                      order of k_pp_ex_repre, pp_cov_top) and their frames
// No FMA is written (the library is built with -ffp-contract=off).

namespace mc {

constexpr int kProjBadIndex = 1, kProjBadOffsets = 2;  // k_proj_validate's flag bits
constexpr int kProjAccWords = 6;                       // ints of one ProjAcc

static_assert(sizeof(ProjAcc) == kProjAccWords * sizeof(int), "ProjAcc is read and written as six ints");

__global__ __launch_bounds__(256) void k_proj_validate(int64_t P, int K, const int64_t *__restrict__ off, int64_t npts,
                                                       const int *__restrict__ pts, int F, int nreq,
                                                       const int *__restrict__ robj, const int *__restrict__ rframe,
                                                       int *__restrict__ flag)
{
    const int64_t n = max(max(npts, static_cast<int64_t>(K) + 1), static_cast<int64_t>(nreq));
    int bad = 0, mx = 0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
        if (i < npts) {
            const int q = pts[i];
            if (q < 0 || q >= P) bad |= kProjBadIndex;
        }
        if (i <= K) {
            const int64_t o = off[i];
            if ((i == 0 && o != 0) || (i == K && o != npts) || o < 0 || o > npts) bad |= kProjBadOffsets;
            if (i < K && off[i + 1] < o) bad |= kProjBadOffsets;
        }
        if (i < nreq) {
            const int o = robj[i], f = rframe[i];
            if (o < 0 || o >= K || f < 0 || f >= F) bad |= kProjBadIndex;
            else mx = max(mx, static_cast<int>(min(max(off[o + 1] - off[o], static_cast<int64_t>(0)), static_cast<int64_t>(INT_MAX))));
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        bad |= __shfl_xor(bad, d, 64);
        mx = max(mx, __shfl_xor(mx, d, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicOr(&flag[0], bad);
        atomicMax(&flag[1], mx);
    }
}

__global__ __launch_bounds__(256) void k_proj_init(int n, int *__restrict__ acc)
{
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        ProjAcc a;
        proj_acc_init(&a);
        int *w = acc + static_cast<int64_t>(j) * kProjAccWords;
        w[0] = a.x0, w[1] = a.y0, w[2] = a.x1, w[3] = a.y1, w[4] = a.inside, w[5] = a.front;
    }
}

// Group g = blockIdx.x: object gobj[g] (g itself without gobj) and the requests goff[g] .. goff[g + 1)
// (g * stride .. + stride without goff; at most kProjMaxTop) of the grouped lists rframe (a negative
// frame: a padded request, skipped) and rout (the request's accumulator; the list position itself
// without rout).  The object's points are cut in turns of kProjChunk; part blockIdx.y takes every
// gridDim.y-th turn, so an object with several turns is served by several workgroups, which combine
// in the pre-initialised accumulator with integer atomics (min, max, add, or: any order gives the
// same words); an object with one turn is written with plain stores.  Per thread: the accumulators
// of all the group's frames in registers; each point's id and coordinates are read once for all of
// them.  The frames' matrices and intrinsics are addressed uniformly (scalar loads).
__global__ __launch_bounds__(256) void k_proj_accum(const int *__restrict__ gobj, const int *__restrict__ goff, int stride,
                                                    const int *__restrict__ rframe, const int *__restrict__ rout,
                                                    const int64_t *__restrict__ opoff, const int *__restrict__ opts,
                                                    const double *__restrict__ pts, const double *__restrict__ intr,
                                                    const double *__restrict__ w2c, int width, int height,
                                                    int *__restrict__ acc)
{
    __shared__ int red[4][kProjMaxTop][kProjAccWords];
    const int g = blockIdx.x;
    const int o = gobj ? gobj[g] : g;
    const int r0 = goff ? goff[g] : g * stride;
    const int nr = min(goff ? goff[g + 1] - r0 : stride, kProjMaxTop);
    const int64_t a = opoff[o], n = opoff[o + 1] - a;
    const int64_t turns = (n + kProjChunk - 1) / kProjChunk;
    if (static_cast<int64_t>(blockIdx.y) >= turns) return;  // (uniform) also an object without points
    const bool shared_acc = turns > 1 && gridDim.y > 1;

    int fr[kProjMaxTop];
    ProjAcc t[kProjMaxTop];
#pragma unroll
    for (int r = 0; r < kProjMaxTop; r++) {
        fr[r] = r < nr ? rframe[r0 + r] : -1;
        proj_acc_init(&t[r]);
    }
    for (int64_t c = blockIdx.y; c < turns; c += gridDim.y) {
        const int64_t e = min(n, (c + 1) * kProjChunk);
        for (int64_t i = c * kProjChunk + threadIdx.x; i < e; i += 256) {
            const int64_t p = opts[a + i];
            const double x = pts[3 * p], y = pts[3 * p + 1], z = pts[3 * p + 2];
#pragma unroll
            for (int r = 0; r < kProjMaxTop; r++) {
                if (fr[r] < 0) continue;  // uniform
                int px = 0, py = 0;
                const int kind = proj_point(w2c + static_cast<int64_t>(fr[r]) * 16, intr + static_cast<int64_t>(fr[r]) * 4, x, y,
                                            z, width, height, &px, &py);
                proj_acc_add(&t[r], kind, px, py);
            }
        }
    }
    // across the wave, then across the four waves through LDS
    const int lane = lane_id(), wv = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < kProjMaxTop; r++) {
        if (fr[r] < 0) continue;
        const int x0 = wave_min_i(t[r].x0), y0 = wave_min_i(t[r].y0), x1 = wave_max_i(t[r].x1), y1 = wave_max_i(t[r].y1);
        const int ins = wave_sum(t[r].inside), front = wave_max_i(t[r].front);
        if (lane == 0) {
            int *w = red[wv][r];
            w[0] = x0, w[1] = y0, w[2] = x1, w[3] = y1, w[4] = ins, w[5] = front;
        }
    }
    __syncthreads();
    const int r = threadIdx.x;
    if (r >= nr || rframe[r0 + r] < 0) return;
    int v[kProjAccWords];
    for (int k = 0; k < kProjAccWords; k++) v[k] = red[0][r][k];
    for (int w = 1; w < 4; w++) {
        v[0] = min(v[0], red[w][r][0]), v[1] = min(v[1], red[w][r][1]);
        v[2] = max(v[2], red[w][r][2]), v[3] = max(v[3], red[w][r][3]);
        v[4] += red[w][r][4], v[5] |= red[w][r][5];
    }
    int *out = acc + static_cast<int64_t>(rout ? rout[r0 + r] : r0 + r) * kProjAccWords;
    if (!shared_acc) {
        for (int k = 0; k < kProjAccWords; k++) out[k] = v[k];
    } else {
        atomicMin(&out[0], v[0]), atomicMin(&out[1], v[1]);
        atomicMax(&out[2], v[2]), atomicMax(&out[3], v[3]);
        if (v[4]) atomicAdd(&out[4], v[4]);
        if (v[5]) atomicOr(&out[5], v[5]);
    }
}

// pad (may be null): a request whose pad[j] is negative is written as -1 throughout
__global__ __launch_bounds__(256) void k_proj_finish(int n, const int *__restrict__ acc, const int *__restrict__ pad,
                                                     int *__restrict__ boxes, int *__restrict__ status,
                                                     int *__restrict__ inside)
{
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        const int *w = acc + static_cast<int64_t>(j) * kProjAccWords;
        const ProjAcc a{w[0], w[1], w[2], w[3], w[4], w[5]};
        int32_t b[4];
        int st = proj_acc_box(&a, b), ins = st == kProjOk ? a.inside : 0;
        if (pad && pad[j] < 0) b[0] = b[1] = b[2] = b[3] = st = ins = -1;
        for (int k = 0; k < 4; k++) boxes[4ll * j + k] = b[k];
        status[j] = st;
        if (inside) inside[j] = ins;
    }
}

// the frame column of every mask of the final objects' mask lists, in k_pp_ex_fill's order
__global__ __launch_bounds__(256) void k_proj_ocol(int nfin, const int *__restrict__ fin_obj, const int *__restrict__ fin_node,
                                                   const int64_t *__restrict__ qoff, const int *__restrict__ qobj,
                                                   const int *__restrict__ qcol, const int64_t *__restrict__ omoff,
                                                   int *__restrict__ ocol)
{
    __shared__ int ws[4];
    for (int f = blockIdx.x; f < nfin; f += gridDim.x) {
        const int o = fin_obj[f], k = fin_node[f];
        const int64_t mb = omoff[f], me = omoff[f + 1];
        pp_compact256(qoff[k], qoff[k + 1], qobj, o, ws, [&](int64_t q, int64_t pos) {
            if (mb + pos < me) ocol[mb + pos] = qcol[q];
        });
    }
}

// a wave per final object: mask_list[:top_k] after find_represent_mask's sort, -1 past the end
__global__ __launch_bounds__(256) void k_proj_top_select(int nfin, int top_k, const int64_t *__restrict__ omoff,
                                                         const double *__restrict__ ocov, const int *__restrict__ ocol,
                                                         int *__restrict__ top_pos, int *__restrict__ top_frame)
{
    const int lane = lane_id();
    for (int f = blockIdx.x * 4 + (threadIdx.x >> 6); f < nfin; f += gridDim.x * 4) {
        const int64_t a = omoff[f];
        const int n = static_cast<int>(omoff[f + 1] - a);
        pp_cov_top(ocov + a, n, top_k, lane, [&](int r, int bp) {
            if (lane != 0) return;
            const int64_t j = static_cast<int64_t>(f) * top_k + r;
            top_pos[j] = bp == INT_MAX ? -1 : bp;
            top_frame[j] = bp == INT_MAX ? -1 : ocol[a + bp];
        });
    }
}

}  // namespace mc
