// mc_paint_kernels.inl — the label painter's kernels (mc_labels_paint; host: mc_paint_host.inl, rules and
// bit arithmetic: mc_paint_plan.hpp).  Three launches per round of frames:
//   k_paint_pack   every mask value is read once and becomes one bit (value == 1) of its instance's bit
//                  plane, ceil(H * W / 64) words; the set bits are counted into the instance's area
//   k_paint_plan   one workgroup per frame: selection, order, kept, ids, the kept list in paint order
//   k_paint_image  one thread per 64-pixel word: the kept planes from the last painted to the first,
//                  folded into eight bit-sliced label planes, transposed to 64 label bytes
// Only integers are added by atomics, so no arrival order reaches a result.

namespace mc {

// the 16 bits of 16 consecutive values at v (16-byte aligned; all in range)
__device__ __forceinline__ uint32_t paint_bits16(const unsigned char *v)
{
    const uint4 q = *reinterpret_cast<const uint4 *>(v);
    return paint_bits4_u8(q.x) | (paint_bits4_u8(q.y) << 4) | (paint_bits4_u8(q.z) << 8) | (paint_bits4_u8(q.w) << 12);
}

__device__ __forceinline__ uint32_t paint_bits16(const float *v)
{
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float4 q = reinterpret_cast<const float4 *>(v)[k];
        bits |= (static_cast<uint32_t>(q.x == 1.0f) | (static_cast<uint32_t>(q.y == 1.0f) << 1) |
                 (static_cast<uint32_t>(q.z == 1.0f) << 2) | (static_cast<uint32_t>(q.w == 1.0f) << 3))
                << (4 * k);
    }
    return bits;
}

__device__ __forceinline__ bool paint_is_one(unsigned char v) { return v == 1; }
__device__ __forceinline__ bool paint_is_one(float v) { return v == 1.0f; }

// grid (x, instances of the launch), 256 threads.  Instance n's values start at masks + n * hw, its
// plane at planes + n * words.  A wave takes 1024 consecutive pixels per step: with a 16-byte aligned
// plane every lane loads its 16 values at once and four lanes' bits make a word; a plane that is
// not aligned (hw no multiple of 16, or such a base) is read one value per lane, a ballot per word.
// Pixels past hw are never read and their bits are zero.
template <typename T>
__global__ __launch_bounds__(256) void k_paint_pack(const T *__restrict__ masks, int64_t hw, int64_t words,
                                                    unsigned long long *__restrict__ planes, int *__restrict__ area)
{
    const int64_t n = blockIdx.y;
    const T *v = masks + n * hw;
    unsigned long long *plane = planes + n * words;
    const int lane = threadIdx.x & 63;
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * 4;
    const bool aligned = (reinterpret_cast<uintptr_t>(v) & 15) == 0;  // the same for every lane of the grid row
    int count = 0;
    for (int64_t base = wave * kPaintWavePixels; base < hw; base += nwaves * kPaintWavePixels) {  // wave-uniform
        if (aligned) {
            const int64_t p = base + lane * kPaintLanePixels;
            uint32_t bits = 0;
            if (p + kPaintLanePixels <= hw) {
                bits = paint_bits16(v + p);
            } else {
                for (int k = 0; k < kPaintLanePixels; k++)
                    if (p + k < hw && paint_is_one(v[p + k])) bits |= 1u << k;
            }
            count += __popc(bits);
            const uint32_t b1 = __shfl_down(bits, 1), b2 = __shfl_down(bits, 2), b3 = __shfl_down(bits, 3);
            const int64_t w = base / 64 + (lane >> 2);
            if ((lane & 3) == 0 && w < words)
                plane[w] = static_cast<unsigned long long>(bits | (b1 << 16)) |
                           (static_cast<unsigned long long>(b2 | (b3 << 16)) << 32);
        } else {
            for (int j = 0; j < kPaintLanePixels; j++) {
                const int64_t p = base + j * 64 + lane;
                if (base + j * 64 >= hw) break;  // wave-uniform
                const unsigned long long word = __ballot(p < hw && paint_is_one(v[p < hw ? p : 0]));
                if (lane == 0) {
                    plane[p / 64] = word;
                    count += __popcll(word);
                }
            }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) count += __shfl_down(count, d);
    if (lane == 0 && count) atomicAdd(area + n, count);
}

// one workgroup of 256 threads per frame (blockIdx.x + frame0).  Instances inst_off[f] .. inst_off[f + 1])
// of the call; `order` gets the frame's kept instances (indices within the frame) from the last painted
// to the first, at the frame's instance offset.  label_instance may be null.
__global__ __launch_bounds__(256) void k_paint_plan(int frame0, const long long *__restrict__ inst_off,
                                                    const float *__restrict__ scores, const int *__restrict__ area,
                                                    float threshold, int min_pixels, int *__restrict__ order,
                                                    int *__restrict__ num_kept, int *__restrict__ status,
                                                    int *__restrict__ label_instance)
{
    __shared__ float s_score[kPaintMaxInstances];
    __shared__ unsigned char s_kept[kPaintMaxInstances];
    __shared__ int s_count;
    const int f = frame0 + blockIdx.x;
    const long long i0 = inst_off[f];
    const int n = static_cast<int>(inst_off[f + 1] - i0);
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float s = scores[i0 + i];
        const bool kept = paint_selected(s, threshold) && area[i0 + i] >= min_pixels;
        s_score[i] = s;
        s_kept[i] = kept;
        mine += kept;
    }
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    const int nk = s_count;
    const bool ok = nk <= kPaintMaxIds;
    if (threadIdx.x == 0) {
        num_kept[f] = nk;
        status[f] = ok ? MC_PAINT_OK : MC_PAINT_OVERFLOW;
    }
    if (label_instance)  // the entries past the ids in use (an overflowing frame uses none)
        for (int k = (ok ? nk : 0) + threadIdx.x; k < kPaintMaxIds; k += 256)
            label_instance[static_cast<long long>(f) * kPaintMaxIds + k] = -1;
    if (!ok) return;
    for (int i = threadIdx.x; i < n; i += 256) {
        if (!s_kept[i]) continue;
        const float si = s_score[i];
        int before = 0;  // kept instances painted before i: its id is before + 1
        for (int j = 0; j < n; j++) before += s_kept[j] && paint_before(s_score[j], j, si, i);
        order[i0 + (nk - 1 - before)] = i;
        if (label_instance) label_instance[static_cast<long long>(f) * kPaintMaxIds + before] = i;
    }
}

// grid (x, frames of the round), 256 threads, one 64-pixel word per thread and step.  plane_inst0: the
// call's instance index of the round's first plane.
__global__ __launch_bounds__(256) void k_paint_image(int frame0, const long long *__restrict__ inst_off, long long plane_inst0,
                                                     int64_t hw, int64_t words,
                                                     const unsigned long long *__restrict__ planes,
                                                     const int *__restrict__ order, const int *__restrict__ num_kept,
                                                     const int *__restrict__ status, unsigned char *__restrict__ labels)
{
    const int f = frame0 + blockIdx.y;
    const long long i0 = inst_off[f];
    const int nk = status[f] == MC_PAINT_OK ? num_kept[f] : 0;
    const int *ord = order + i0;
    const unsigned long long *fplanes = planes + (i0 - plane_inst0) * words;
    unsigned char *img = labels + static_cast<int64_t>(f) * hw;
    const bool aligned = (reinterpret_cast<uintptr_t>(img) & 15) == 0;
    for (int64_t w = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; w < words; w += static_cast<int64_t>(gridDim.x) * 256) {
        const int64_t left = hw - w * 64;  // pixels of this word, 64 but for the last
        uint64_t done = left >= 64 ? 0ull : ~0ull << left;
        uint64_t lab[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < nk && done != ~0ull; k++) {
            const uint64_t newly = fplanes[ord[k] * words + w] & ~done;
            paint_fold(lab, newly, nk - k);
            done |= newly;
        }
        unsigned char *o = img + w * 64;
        if (aligned && left >= 64) {
#pragma unroll
            for (int g = 0; g < 8; g += 2) {
                const uint64_t a = paint_label_bytes(lab, g), b = paint_label_bytes(lab, g + 1);
                uint4 q;
                q.x = static_cast<uint32_t>(a), q.y = static_cast<uint32_t>(a >> 32);
                q.z = static_cast<uint32_t>(b), q.w = static_cast<uint32_t>(b >> 32);
                *reinterpret_cast<uint4 *>(o + 8 * g) = q;
            }
        } else {
            for (int g = 0; g < 8 && 8 * g < left; g++) {
                const uint64_t a = paint_label_bytes(lab, g);
                for (int p = 0; p < 8 && 8 * g + p < left; p++) o[8 * g + p] = static_cast<unsigned char>(a >> (8 * p));
            }
        }
    }
}

}  // namespace mc
