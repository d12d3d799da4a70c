// mc_crop_host.inl — host driver of the CLIP crop preparation (mc_crop_*; kernels: mc_crop_kernels.inl,
// arithmetic: mc_crop_plan.hpp).  Included by mc_api.hip after the context is defined.
//
// mask_frame / mask_label are host arrays in both calls: they are range-checked before anything is
// launched.  Frames given on the host are uploaded compactly (only the referenced ones); boxes and
// status may stay on the device between mc_crop_boxes and mc_crop_render, and then neither call
// waits for the stream.

namespace {

constexpr int kCropMaxOut = 4096, kCropMaxLevels = 16;
constexpr int64_t kCropDefaultBudget = 1ll << 30;  // scratch bytes of one render launch without a budget set

void crop_check_params(const mc_crop_params *p)
{
    MC_REQUIRE(p, MC_ERR_INVALID, "null crop parameters");
    MC_REQUIRE(p->out_size >= 1 && p->out_size <= kCropMaxOut, MC_ERR_INVALID, "out_size outside [1, 4096]");
    MC_REQUIRE(p->levels >= 1 && p->levels <= kCropMaxLevels, MC_ERR_INVALID, "levels outside [1, 16]");
    MC_REQUIRE(p->expansion >= 0.0 && p->expansion <= 1e6, MC_ERR_INVALID, "expansion outside [0, 1e6]");
}

void crop_check_frames(int32_t num_frames, int32_t H, int32_t W, int32_t num_masks)
{
    MC_REQUIRE(num_frames >= 0 && num_masks >= 0, MC_ERR_INVALID, "negative size");
    MC_REQUIRE(H >= 1 && W >= 1 && static_cast<int64_t>(H) * W <= (1ll << 30), MC_ERR_INVALID, "bad frame size");
}

// the distinct frames of mask_frame in order of first use and every mask's slot among them
void crop_frame_slots(int32_t num_frames, int32_t n, const int32_t *mask_frame, std::vector<int32_t> &frames,
                      std::vector<int32_t> &slot)
{
    std::vector<int32_t> of(num_frames, -1);
    frames.clear();
    slot.resize(n);
    for (int m = 0; m < n; m++) {
        int32_t &s = of[mask_frame[m]];
        if (s < 0) {
            s = static_cast<int32_t>(frames.size());
            frames.push_back(mask_frame[m]);
        }
        slot[m] = s;
    }
}

// host frames: the referenced ones, packed in slot order (frames[] becomes the identity)
const unsigned char *crop_upload_frames(mc_ctx *ctx, DevBuf &buf, const uint8_t *src, int64_t frame_bytes,
                                        std::vector<int32_t> &frames)
{
    buf.reserve(frames.size() * frame_bytes + 8);
    for (size_t k = 0; k < frames.size(); k++) {
        MC_HIP(hipMemcpyAsync(buf.as<unsigned char>() + k * frame_bytes, src + frames[k] * frame_bytes, frame_bytes,
                              hipMemcpyHostToDevice, ctx->stream));
        frames[k] = static_cast<int32_t>(k);
    }
    return buf.as<unsigned char>();
}

}  // namespace

extern "C" {

void mc_crop_params_default(mc_crop_params *p)
{
    if (!p) return;
    p->out_size = 224;
    p->levels = 3;       // CROP_SCALES (get_open-voc_features.py:18)
    p->expansion = 0.1;  // :66
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, sd[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    for (int c = 0; c < 3; c++) p->mean[c] = mean[c], p->std[c] = sd[c], p->pad_rgb[c] = 255;  // :78
}

int mc_crop_boxes(mc_ctx *ctx, int32_t num_frames, int32_t H, int32_t W, const uint8_t *seg, int on_device,
                  int32_t num_masks, const int32_t *mask_frame, const int32_t *mask_label, const mc_crop_params *params,
                  int32_t *boxes, int32_t *status, int out_on_device)
{
    return guarded(ctx, [&] {
        crop_check_params(params);
        crop_check_frames(num_frames, H, W, num_masks);
        if (!num_masks) return;
        MC_REQUIRE(seg && mask_frame && mask_label && boxes && status, MC_ERR_INVALID, "null argument");
        for (int m = 0; m < num_masks; m++) {
            MC_REQUIRE(mask_frame[m] >= 0 && mask_frame[m] < num_frames, MC_ERR_INVALID, "mask frame index out of range");
            MC_REQUIRE(mask_label[m] >= 0 && mask_label[m] <= 255, MC_ERR_INVALID, "mask label outside [0, 255]");
        }
        CropState &c = ctx->crop;
        hipStream_t s = ctx->stream;
        const int n = num_masks, L = params->levels;
        crop_frame_slots(num_frames, n, mask_frame, c.h_frames, c.h_slot);
        c.h_label.assign(mask_label, mask_label + n);
        const int nref = static_cast<int>(c.h_frames.size());
        const unsigned char *dseg = on_device ? seg : crop_upload_frames(ctx, c.in_seg, seg, static_cast<int64_t>(H) * W, c.h_frames);
        c.frames.reserve(nref * 4);
        c.slot.reserve(n * 4);
        c.label.reserve(n * 4);
        c.tab.reserve(static_cast<size_t>(nref) * 1024 * 4);
        MC_HIP(hipMemcpyAsync(c.frames.ptr, c.h_frames.data(), nref * 4, hipMemcpyHostToDevice, s));
        MC_HIP(hipMemcpyAsync(c.slot.ptr, c.h_slot.data(), n * 4, hipMemcpyHostToDevice, s));
        MC_HIP(hipMemcpyAsync(c.label.ptr, c.h_label.data(), n * 4, hipMemcpyHostToDevice, s));
        int *dbox = boxes, *dstat = status;
        if (!out_on_device) {
            c.out_boxes.reserve(static_cast<size_t>(n) * L * 16);
            c.out_status.reserve(n * 4);
            dbox = c.out_boxes.as<int>(), dstat = c.out_status.as<int>();
        }
        {
            TimedScope ts(ctx->timer, s, "crop_boxes");
            hipLaunchKernelGGL(mc::k_crop_table_init, grid_for(nref * 1024ll, 256, 1 << 30), dim3(256), 0, s, nref * 1024,
                               c.tab.as<int>());
            const int words = (H * W + 3) / 4;
            const int gx = std::max(1, std::min(64, ceil_div(words, 256 * 8)));
            for (int f0 = 0; f0 < nref; f0 += 32768)
                hipLaunchKernelGGL(mc::k_crop_frame_boxes, dim3(gx, std::min(32768, nref - f0)), dim3(256), 0, s, dseg, H, W,
                                   c.frames.as<int>(), f0, c.tab.as<int>());
            hipLaunchKernelGGL(mc::k_crop_mask_boxes, grid_for(n, 256, 1 << 30), dim3(256), 0, s, n, c.slot.as<int>(),
                               c.label.as<int>(), c.tab.as<int>(), H, W, L, params->expansion, dbox, dstat);
            MC_HIP(hipGetLastError());
        }
        if (!out_on_device) {
            MC_HIP(hipMemcpyAsync(boxes, dbox, static_cast<size_t>(n) * L * 16, hipMemcpyDeviceToHost, s));
            fetch(ctx, status, dstat, n * 4);
            ctx->timer.collect();
        }
    });
}

int mc_crop_render(mc_ctx *ctx, int32_t num_frames, int32_t H, int32_t W, const uint8_t *rgb, int on_device,
                   int32_t num_masks, const int32_t *mask_frame, const int32_t *boxes, const int32_t *status,
                   int boxes_on_device, const mc_crop_params *params, float *out)
{
    return guarded(ctx, [&] {
        crop_check_params(params);
        crop_check_frames(num_frames, H, W, num_masks);
        if (!num_masks) return;
        MC_REQUIRE(rgb && mask_frame && boxes && status && out, MC_ERR_INVALID, "null argument");
        const int n = num_masks, L = params->levels, S = params->out_size;
        for (int m = 0; m < n; m++)
            MC_REQUIRE(mask_frame[m] >= 0 && mask_frame[m] < num_frames, MC_ERR_INVALID, "mask frame index out of range");
        if (!boxes_on_device)
            for (int m = 0; m < n; m++) {
                MC_REQUIRE(status[m] >= mc::kCropOk && status[m] <= mc::kCropEmpty, MC_ERR_INVALID, "unknown mask status");
                for (int lv = 0; lv < L && status[m] == mc::kCropOk; lv++) {
                    const int32_t *b = boxes + (static_cast<int64_t>(m) * L + lv) * 4;
                    MC_REQUIRE(b[0] >= 0 && b[0] <= b[2] && b[2] <= W && b[1] >= 0 && b[1] <= b[3] && b[3] <= H, MC_ERR_INVALID,
                               "crop box outside its frame");
                }
            }
        // scratch of one crop: the uint8 intermediate of the largest square, its table and bounds
        const int maxhw = std::max(H, W), kmax = mc::crop_max_ksize(H, W, S);
        const int64_t tmp_stride = static_cast<int64_t>(maxhw) * S * 3;
        const int64_t per_mask = L * (tmp_stride + static_cast<int64_t>(kmax) * S * 4 + S * 8ll);
        const int64_t budget = ctx->bp.mem_budget ? ctx->bp.mem_budget : kCropDefaultBudget;
        MC_REQUIRE(per_mask <= budget, MC_ERR_UNSUPPORTED, "one mask's crop scratch exceeds the memory budget");
        const int sub = static_cast<int>(std::min<int64_t>(std::min<int64_t>(n, 65535 / L), budget / per_mask));

        CropState &c = ctx->crop;
        hipStream_t s = ctx->stream;
        c.h_mframe.assign(mask_frame, mask_frame + n);
        const unsigned char *drgb = rgb;
        if (!on_device) {
            crop_frame_slots(num_frames, n, mask_frame, c.h_frames, c.h_mframe);
            drgb = crop_upload_frames(ctx, c.in_rgb, rgb, static_cast<int64_t>(H) * W * 3, c.h_frames);
        }
        c.mframe.reserve(n * 4);
        MC_HIP(hipMemcpyAsync(c.mframe.ptr, c.h_mframe.data(), n * 4, hipMemcpyHostToDevice, s));
        const int *dbox = boxes, *dstat = status;
        if (!boxes_on_device) {
            c.in_boxes.reserve(static_cast<size_t>(n) * L * 16);
            c.in_status.reserve(n * 4);
            MC_HIP(hipMemcpyAsync(c.in_boxes.ptr, boxes, static_cast<size_t>(n) * L * 16, hipMemcpyHostToDevice, s));
            MC_HIP(hipMemcpyAsync(c.in_status.ptr, status, n * 4, hipMemcpyHostToDevice, s));
            dbox = c.in_boxes.as<int>(), dstat = c.in_status.as<int>();
        }
        // ((float32(v) / 255f) - mean) / std in float32 (ToTensor, Normalize), as a table
        c.h_lut.resize(768);
        for (int ch = 0; ch < 3; ch++)
            for (int v = 0; v < 256; v++) {
                const float x = static_cast<float>(v) / 255.0f;
                const float d = x - params->mean[ch];
                c.h_lut[ch * 256 + v] = d / params->std[ch];
            }
        c.lut.reserve(768 * 4);
        MC_HIP(hipMemcpyAsync(c.lut.ptr, c.h_lut.data(), 768 * 4, hipMemcpyHostToDevice, s));
        c.tmp.reserve(static_cast<size_t>(sub) * L * tmp_stride);
        c.kk.reserve(static_cast<size_t>(sub) * L * kmax * S * 4);
        c.bounds.reserve(static_cast<size_t>(sub) * L * S * 8);
        const int64_t plane = static_cast<int64_t>(S) * S;
        for (int m0 = 0; m0 < n; m0 += sub) {
            const int nm = std::min(sub, n - m0), nc = nm * L;
            const int *bx = dbox + static_cast<int64_t>(m0) * L * 4, *st = dstat + m0;
            const int gh = static_cast<int>(std::max<int64_t>(8, std::min<int64_t>(2048 / nc, ceil_div(static_cast<int64_t>(maxhw) * S, 256))));
            const int gv = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(std::max(4, 2048 / nc), ceil_div(plane, 256))));
            {
                TimedScope ts(ctx->timer, s, "crop_coeffs");
                hipLaunchKernelGGL(mc::k_crop_coeffs, dim3(ceil_div(S, 256), nc), dim3(256), 0, s, bx, st, L, H, W, S, kmax,
                                   c.bounds.as<int>(), c.kk.as<int>());
            }
            {
                TimedScope ts(ctx->timer, s, "crop_h");
                hipLaunchKernelGGL(mc::k_crop_h, dim3(gh, nc), dim3(256), 0, s, drgb, H, W, c.mframe.as<int>() + m0, bx, st, L, S,
                                   kmax, c.bounds.as<int>(), c.kk.as<int>(), static_cast<int>(params->pad_rgb[0]),
                                   static_cast<int>(params->pad_rgb[1]), static_cast<int>(params->pad_rgb[2]), tmp_stride,
                                   c.tmp.as<unsigned char>());
            }
            {
                TimedScope ts(ctx->timer, s, "crop_v");
                hipLaunchKernelGGL(mc::k_crop_v, dim3(gv, nc), dim3(256), 0, s, bx, st, L, H, W, S, kmax, c.bounds.as<int>(),
                                   c.kk.as<int>(), tmp_stride, c.tmp.as<unsigned char>(), c.lut.as<float>(),
                                   out + static_cast<int64_t>(m0) * L * 3 * plane);
            }
            MC_HIP(hipGetLastError());
        }
    });
}

int mc_crop_coeffs(mc_ctx *ctx, int32_t in_size, int32_t out_size, int32_t *ksize, int32_t *bounds, int32_t *kk)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ksize, MC_ERR_INVALID, "null argument");
        MC_REQUIRE(in_size >= 1 && in_size <= (1 << 24) && out_size >= 1 && out_size <= kCropMaxOut, MC_ERR_INVALID,
                   "in_size outside [1, 2^24] or out_size outside [1, 4096]");
        const int K = mc::crop_ksize(in_size, out_size), S = out_size;
        *ksize = K;
        if (!bounds && !kk) return;  // the size query
        MC_REQUIRE(bounds && kk, MC_ERR_INVALID, "null argument");
        MC_REQUIRE(static_cast<int64_t>(K) * S <= (1ll << 26), MC_ERR_UNSUPPORTED, "coefficient table above 2^26 entries");
        CropState &c = ctx->crop;
        hipStream_t s = ctx->stream;
        c.bounds.reserve(S * 8);
        c.kk.reserve(static_cast<size_t>(K) * S * 4);
        {
            TimedScope ts(ctx->timer, s, "crop_coeffs");
            hipLaunchKernelGGL(mc::k_crop_coeffs_table, dim3(ceil_div(S, 256)), dim3(256), 0, s, in_size, S, K, c.bounds.as<int>(),
                               c.kk.as<int>());
            MC_HIP(hipGetLastError());
        }
        MC_HIP(hipMemcpyAsync(bounds, c.bounds.ptr, S * 8, hipMemcpyDeviceToHost, s));
        fetch(ctx, kk, c.kk.ptr, static_cast<size_t>(K) * S * 4);
        ctx->timer.collect();
    });
}

}  // extern "C"
