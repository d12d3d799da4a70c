// mc_crop_kernels.inl — CLIP crop preparation on the device (semantics/get_open-voc_features.py:44-99).
//
// Boxes: k_crop_frame_boxes reads every referenced segmentation frame once, whatever the number of
// labels asked of it, and keeps per workgroup a 256-label table of (min x, max x, min y, max y) in
// LDS (4 KiB); a wave whose 256 pixels all carry one label reduces its bounds with shuffles and makes
// four LDS atomics, any other wave makes them per run of equal pixels.  The tables merge into one
// per frame with global atomics; k_crop_mask_boxes turns them into the level boxes and the status.
//
// Render: three launches for a whole chunk of crops (grid.y = crop).  k_crop_coeffs computes each
// crop's coefficient table from mc_crop_plan.hpp, one thread per output index, stored tap-major
// (tap j of output xx at j * S + xx) so that neighbouring threads read neighbouring words in both
// passes.  k_crop_h is Pillow's horizontal pass over the virtual white square (a tap outside the
// pasted crop reads the pad colour; the square is never stored) into the uint8 intermediate
// [s, S, 3]; k_crop_v is the vertical pass, the 3 x 256 normalisation table and the channel-first
// float32 store.  A square of side S passes through both unchanged, as Image.resize returns a copy.
//
// Bounds: a crop's intermediate lives at crop * max(H, W) * S * 3 bytes of the scratch buffer and its
// table at crop * kmax * S words with kmax = crop_ksize(max(H, W), S); a box is rendered only when
// 0 <= left <= right <= W and 0 <= top <= bottom <= H, so s <= max(H, W), a row's taps <= kmax, and
// every source pixel read lies inside its frame.  No kernel uses LDS beyond the 4 KiB label table.

namespace mc {

__global__ __launch_bounds__(256) void k_crop_table_init(int n, int *__restrict__ tab)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) tab[i] = (i & 1) ? -1 : 0x7fffffff;  // (min x, max x, min y, max y)
}

__device__ __forceinline__ void crop_lds_bounds(int *t, int lab, int x0, int x1, int y0, int y1)
{
    atomicMin(&t[lab * 4 + 0], x0);
    atomicMax(&t[lab * 4 + 1], x1);
    atomicMin(&t[lab * 4 + 2], y0);
    atomicMax(&t[lab * 4 + 3], y1);
}

// grid (blocks per frame, frames of this launch): frame slot = slot0 + blockIdx.y, its pixels at
// seg + frames[slot] * H * W, its table at tab + slot * 1024
__global__ __launch_bounds__(256) void k_crop_frame_boxes(const unsigned char *__restrict__ seg, int H, int W,
                                                          const int *__restrict__ frames, int slot0, int *__restrict__ tab)
{
    __shared__ int t[256 * 4];
    const int tid = threadIdx.x;
    t[tid * 4 + 0] = 0x7fffffff, t[tid * 4 + 1] = -1, t[tid * 4 + 2] = 0x7fffffff, t[tid * 4 + 3] = -1;
    __syncthreads();
    const int slot = slot0 + blockIdx.y;
    const int plane = H * W;
    const unsigned char *base = seg + static_cast<int64_t>(frames[slot]) * plane;
    const bool aligned = (reinterpret_cast<uintptr_t>(base) & 3u) == 0;
    const int words = (plane + 3) >> 2;
    for (int start = blockIdx.x * 256; start < words; start += gridDim.x * 256) {  // the same trips in every lane
        const int wi = start + tid;
        const int p0 = wi * 4;
        const int nv = wi < words ? min(4, plane - p0) : 0;
        unsigned v = 0;
        if (nv == 4 && aligned) {
            v = *reinterpret_cast<const unsigned *>(base + p0);
        } else {
            for (int j = 0; j < nv; j++) v |= static_cast<unsigned>(base[p0 + j]) << (8 * j);
        }
        const int y0 = nv ? p0 / W : 0, x0 = nv ? p0 - y0 * W : 0;
        const int lab0 = v & 255;
        const bool single = nv == 4 && v == lab0 * 0x01010101u && x0 + 3 < W;
        const int first = __shfl(lab0, 0);
        if (__all(single && lab0 == first)) {
            int a = x0, b = x0 + 3, c = y0, d = y0;
            for (int o = 32; o; o >>= 1) {
                a = min(a, __shfl_xor(a, o));
                b = max(b, __shfl_xor(b, o));
                c = min(c, __shfl_xor(c, o));
                d = max(d, __shfl_xor(d, o));
            }
            if ((tid & 63) == 0) crop_lds_bounds(t, first, a, b, c, d);
        } else if (single) {
            crop_lds_bounds(t, lab0, x0, x0 + 3, y0, y0);
        } else {
            int x = x0, y = y0;
            for (int j = 0; j < nv; j++) {
                crop_lds_bounds(t, (v >> (8 * j)) & 255, x, x, y, y);
                if (++x == W) x = 0, y++;
            }
        }
    }
    __syncthreads();
    if (t[tid * 4 + 1] >= 0) {
        int *g = tab + (static_cast<int64_t>(slot) * 256 + tid) * 4;
        atomicMin(&g[0], t[tid * 4 + 0]);
        atomicMax(&g[1], t[tid * 4 + 1]);
        atomicMin(&g[2], t[tid * 4 + 2]);
        atomicMax(&g[3], t[tid * 4 + 3]);
    }
}

__global__ __launch_bounds__(256) void k_crop_mask_boxes(int n, const int *__restrict__ mask_slot,
                                                         const int *__restrict__ mask_label, const int *__restrict__ tab, int H,
                                                         int W, int levels, double expansion, int *__restrict__ boxes,
                                                         int *__restrict__ status)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= n) return;
    const int *g = tab + (static_cast<int64_t>(mask_slot[m]) * 256 + mask_label[m]) * 4;
    const int left = g[0], right = g[1], top = g[2], bottom = g[3];
    int *b = boxes + static_cast<int64_t>(m) * levels * 4;
    if (right < 0) {
        status[m] = kCropAbsent;
        for (int i = 0; i < levels * 4; i++) b[i] = 0;
        return;
    }
    status[m] = (left == right && top == bottom) ? kCropEmpty : kCropOk;
    for (int lv = 0; lv < levels; lv++) crop_level_box(left, top, right, bottom, H, W, lv, expansion, b + lv * 4);
}

// the square of crop `crop` (mask crop / levels), or false when nothing is rendered for it
__device__ __forceinline__ bool crop_load(const int *__restrict__ boxes, const int *__restrict__ status, int crop, int levels,
                                          int H, int W, int box[4], CropSquare &q)
{
    if (status[crop / levels] != kCropOk) return false;
    for (int i = 0; i < 4; i++) box[i] = boxes[static_cast<int64_t>(crop) * 4 + i];
    if (box[0] < 0 || box[0] > box[2] || box[2] > W || box[1] < 0 || box[1] > box[3] || box[3] > H) return false;
    q = crop_square(box);
    return q.s > 0;
}

// grid (ceil(S / 256), crops): bounds [crop][S][2] = (first tap, taps), kk [crop][kmax][S]
__global__ __launch_bounds__(256) void k_crop_coeffs(const int *__restrict__ boxes, const int *__restrict__ status, int levels,
                                                     int H, int W, int S, int kmax, int *__restrict__ bounds,
                                                     int *__restrict__ kk)
{
    const int crop = blockIdx.y, xx = blockIdx.x * 256 + threadIdx.x;
    int box[4];
    CropSquare q;
    if (xx >= S || !crop_load(boxes, status, crop, levels, H, W, box, q) || q.s == S) return;
    int32_t xmin;
    const int n = crop_coeff_row(q.s, S, xx, &xmin, kk + static_cast<int64_t>(crop) * kmax * S + xx, S);
    bounds[(static_cast<int64_t>(crop) * S + xx) * 2 + 0] = xmin;
    bounds[(static_cast<int64_t>(crop) * S + xx) * 2 + 1] = n;
}

// one (in_size, out_size) table in Pillow's layout (mc_crop_coeffs): bounds [S][2], kk [S][ksize], unused taps 0
__global__ __launch_bounds__(256) void k_crop_coeffs_table(int in_size, int S, int ksize, int *__restrict__ bounds,
                                                           int *__restrict__ kk)
{
    const int xx = blockIdx.x * 256 + threadIdx.x;
    if (xx >= S) return;
    int32_t xmin;
    int *row = kk + static_cast<int64_t>(xx) * ksize;
    const int n = crop_coeff_row(in_size, S, xx, &xmin, row, 1);
    for (int j = n; j < ksize; j++) row[j] = 0;
    bounds[xx * 2 + 0] = xmin;
    bounds[xx * 2 + 1] = n;
}

// horizontal pass: grid (blocks per crop, crops); tmp [crop] = uint8 [s, S, 3]
__global__ __launch_bounds__(256) void k_crop_h(const unsigned char *__restrict__ rgb, int H, int W,
                                                const int *__restrict__ mask_frame, const int *__restrict__ boxes,
                                                const int *__restrict__ status, int levels, int S, int kmax,
                                                const int *__restrict__ bounds, const int *__restrict__ kk, int pad_r, int pad_g,
                                                int pad_b, int64_t tmp_stride, unsigned char *__restrict__ tmp)
{
    const int crop = blockIdx.y;
    int box[4];
    CropSquare q;
    if (!crop_load(boxes, status, crop, levels, H, W, box, q)) return;
    const unsigned char *src = rgb + static_cast<int64_t>(mask_frame[crop / levels]) * H * W * 3;
    unsigned char *dst = tmp + crop * tmp_stride;
    const int *cb = bounds + static_cast<int64_t>(crop) * S * 2;
    const int *ck = kk + static_cast<int64_t>(crop) * kmax * S;
    const bool copy = q.s == S;
    const int64_t total = static_cast<int64_t>(q.s) * S;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
        const int y = static_cast<int>(i / S), xx = static_cast<int>(i - static_cast<int64_t>(y) * S);
        const int sy = y - q.oy;
        const bool row_in = sy >= 0 && sy < q.h;
        const unsigned char *row = src + (static_cast<int64_t>(box[1] + (row_in ? sy : 0)) * W + box[0]) * 3;
        int r, g, b;
        if (copy) {
            const int x = xx - q.ox;
            const bool in = row_in && x >= 0 && x < q.w;
            r = in ? row[x * 3 + 0] : pad_r, g = in ? row[x * 3 + 1] : pad_g, b = in ? row[x * 3 + 2] : pad_b;
        } else {
            const int x0 = cb[xx * 2] - q.ox, n = cb[xx * 2 + 1];
            r = g = b = 1 << (kCropPrecisionBits - 1);
            for (int j = 0; j < n; j++) {
                const int k = ck[j * S + xx];
                const int x = x0 + j;
                const bool in = row_in && x >= 0 && x < q.w;
                r += k * (in ? row[x * 3 + 0] : pad_r);
                g += k * (in ? row[x * 3 + 1] : pad_g);
                b += k * (in ? row[x * 3 + 2] : pad_b);
            }
            r = crop_clip8(r), g = crop_clip8(g), b = crop_clip8(b);
        }
        dst[i * 3 + 0] = static_cast<unsigned char>(r);
        dst[i * 3 + 1] = static_cast<unsigned char>(g);
        dst[i * 3 + 2] = static_cast<unsigned char>(b);
    }
}

// vertical pass, normalisation table, channel-first store: out [crop][3][S][S]; a crop that is not
// rendered (status, an invalid box) is written as zeros
__global__ __launch_bounds__(256) void k_crop_v(const int *__restrict__ boxes, const int *__restrict__ status, int levels, int H,
                                                int W, int S, int kmax, const int *__restrict__ bounds,
                                                const int *__restrict__ kk, int64_t tmp_stride,
                                                const unsigned char *__restrict__ tmp, const float *__restrict__ lut,
                                                float *__restrict__ out)
{
    const int crop = blockIdx.y;
    const int64_t plane = static_cast<int64_t>(S) * S;
    float *o = out + static_cast<int64_t>(crop) * 3 * plane;
    int box[4];
    CropSquare q;
    if (!crop_load(boxes, status, crop, levels, H, W, box, q)) {
        for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < 3 * plane; i += gridDim.x * 256ll) o[i] = 0.f;
        return;
    }
    const unsigned char *t = tmp + crop * tmp_stride;
    const int *cb = bounds + static_cast<int64_t>(crop) * S * 2;
    const int *ck = kk + static_cast<int64_t>(crop) * kmax * S;
    const bool copy = q.s == S;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < plane; i += gridDim.x * 256ll) {
        const int yy = static_cast<int>(i / S), xx = static_cast<int>(i - static_cast<int64_t>(yy) * S);
        int r, g, b;
        if (copy) {
            r = t[i * 3 + 0], g = t[i * 3 + 1], b = t[i * 3 + 2];
        } else {
            const int y0 = cb[yy * 2], n = cb[yy * 2 + 1];
            r = g = b = 1 << (kCropPrecisionBits - 1);
            for (int j = 0; j < n; j++) {
                const int k = ck[j * S + yy];
                const unsigned char *p = t + (static_cast<int64_t>(y0 + j) * S + xx) * 3;
                r += k * p[0], g += k * p[1], b += k * p[2];
            }
            r = crop_clip8(r), g = crop_clip8(g), b = crop_clip8(b);
        }
        o[i] = lut[r];
        o[plane + i] = lut[256 + g];
        o[2 * plane + i] = lut[512 + b];
    }
}

}  // namespace mc
