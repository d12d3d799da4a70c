// mc_paint_host.inl — host driver of the label painter (mc_labels_paint; kernels: mc_paint_kernels.inl,
// decisions: mc_paint_plan.hpp).  Included by mc_api.hip after the context is defined.
//
// inst_off is a host array: it and every other argument are checked, and the rounds of frames are
// planned against the scratch budget, before anything is launched or any context state is written.
// A round packs its frames' masks into bit planes (host masks are staged round by round), plans the
// frames and paints them.  Host outputs and host inputs wait for the stream; a call with device inputs
// and device outputs does not.

namespace {

template <typename T>
void paint_pack_launch(mc_ctx *ctx, const void *masks, int64_t ninst, int64_t hw, int64_t words, unsigned long long *planes,
                       int *area)
{
    const int gx = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(256, ceil_div(hw, 4 * mc::kPaintWavePixels))));
    for (int64_t n0 = 0; n0 < ninst; n0 += 32768)
        hipLaunchKernelGGL(mc::k_paint_pack<T>, dim3(gx, static_cast<unsigned>(std::min<int64_t>(32768, ninst - n0))), dim3(256),
                           0, ctx->stream, static_cast<const T *>(masks) + n0 * hw, hw, words, planes + n0 * words, area + n0);
}

// a small output of the call: to the caller's device array, or to the host (waited for by the caller of this)
void paint_deliver(mc_ctx *ctx, void *dst, const void *src, size_t bytes, int out_on_device)
{
    if (dst && bytes)
        MC_HIP(hipMemcpyAsync(dst, src, bytes, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
}

}  // namespace

extern "C" {

void mc_paint_params_default(mc_paint_params *p)
{
    if (!p) return;
    p->score_threshold = 0.5f;  // --confidence-threshold (mask_predict.py:62)
    p->min_pixels = 400;        // :108
}

int mc_labels_paint(mc_ctx *ctx, int32_t num_frames, int32_t H, int32_t W, const int64_t *inst_off, int32_t mask_dtype,
                    const void *masks, const float *scores, int on_device, const mc_paint_params *params,
                    uint8_t *labels_out, int32_t *status, int32_t *num_kept, int32_t *label_instance,
                    int32_t *instance_area, int out_on_device)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(params, MC_ERR_INVALID, "null paint parameters");
        std::string why;
        MC_REQUIRE(mc::paint_check_args(num_frames, H, W, inst_off, mask_dtype, params->min_pixels, &why) == mc::kPaintAccept,
                   MC_ERR_INVALID, why);
        const int F = num_frames;
        if (!F) return;
        const int64_t hw = static_cast<int64_t>(H) * W, words = mc::paint_words(hw), ntot = inst_off[F];
        MC_REQUIRE(labels_out && (ntot == 0 || (masks && scores)), MC_ERR_INVALID, "null argument");
        const bool staged = !on_device;
        const int vb = mc::paint_value_bytes(mask_dtype);
        std::vector<std::pair<int, int>> rounds;
        MC_REQUIRE(mc::paint_rounds(F, inst_off, hw, mask_dtype, staged, mc::paint_byte_budget(ctx->bp.mem_budget), &rounds,
                                    &why) == mc::kPaintAccept,
                   MC_ERR_UNSUPPORTED, why);
        int64_t max_inst = 0;
        for (const auto &r : rounds) max_inst = std::max(max_inst, inst_off[r.second] - inst_off[r.first]);

        PaintState &p = ctx->paint;
        hipStream_t s = ctx->stream;
        p.off.reserve((F + 1) * 8);
        p.area.reserve(ntot * 4 + 8);
        p.order.reserve(ntot * 4 + 8);
        p.kept.reserve(F * 4);
        p.status.reserve(F * 4);
        p.planes.reserve(static_cast<size_t>(max_inst) * words * 8 + 8);
        if (staged) {
            p.stage.reserve(static_cast<size_t>(max_inst) * hw * vb + 8);
            p.scores.reserve(ntot * 4 + 8);
            if (ntot) MC_HIP(hipMemcpyAsync(p.scores.ptr, scores, ntot * 4, hipMemcpyHostToDevice, s));
        }
        const float *dscores = staged ? p.scores.as<float>() : scores;
        int *dlab = label_instance;
        if (label_instance && !out_on_device) {
            p.labinst.reserve(static_cast<size_t>(F) * mc::kPaintMaxIds * 4);
            dlab = p.labinst.as<int>();
        }
        p.h_off.assign(inst_off, inst_off + F + 1);
        MC_HIP(hipMemcpyAsync(p.off.ptr, p.h_off.data(), (F + 1) * 8, hipMemcpyHostToDevice, s));
        MC_HIP(hipMemsetAsync(p.area.ptr, 0, ntot * 4 + 8, s));

        for (const auto &r : rounds) {
            const int f0 = r.first, nf = r.second - r.first;
            const int64_t i0 = inst_off[f0], ninst = inst_off[r.second] - i0;
            const char *dmasks = static_cast<const char *>(masks) + i0 * hw * vb;
            if (staged && ninst) {
                MC_HIP(hipMemcpyAsync(p.stage.ptr, dmasks, ninst * hw * vb, hipMemcpyHostToDevice, s));
                dmasks = p.stage.as<char>();
            }
            if (ninst) {
                TimedScope ts(ctx->timer, s, "paint_pack");
                if (mask_dtype == mc::kPaintF32)
                    paint_pack_launch<float>(ctx, dmasks, ninst, hw, words, p.planes.as<unsigned long long>(), p.area.as<int>() + i0);
                else
                    paint_pack_launch<unsigned char>(ctx, dmasks, ninst, hw, words, p.planes.as<unsigned long long>(),
                                                     p.area.as<int>() + i0);
            }
            {
                TimedScope ts(ctx->timer, s, "paint_plan");
                hipLaunchKernelGGL(mc::k_paint_plan, dim3(nf), dim3(256), 0, s, f0, p.off.as<long long>(), dscores, p.area.as<int>(),
                                   params->score_threshold, params->min_pixels, p.order.as<int>(), p.kept.as<int>(),
                                   p.status.as<int>(), dlab);
            }
            {
                TimedScope ts(ctx->timer, s, "paint_image");
                const int gx = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(4096, ceil_div(words, 256))));
                for (int g0 = 0; g0 < nf; g0 += 32768)
                    hipLaunchKernelGGL(mc::k_paint_image, dim3(gx, std::min(32768, nf - g0)), dim3(256), 0, s, f0 + g0,
                                       p.off.as<long long>(), static_cast<long long>(i0), hw, words,
                                       p.planes.as<unsigned long long>(), p.order.as<int>(), p.kept.as<int>(), p.status.as<int>(),
                                       labels_out);
            }
            MC_HIP(hipGetLastError());
        }
        paint_deliver(ctx, status, p.status.ptr, F * 4, out_on_device);
        paint_deliver(ctx, num_kept, p.kept.ptr, F * 4, out_on_device);
        paint_deliver(ctx, instance_area, p.area.ptr, ntot * 4, out_on_device);
        if (!out_on_device) paint_deliver(ctx, label_instance, dlab, static_cast<size_t>(F) * mc::kPaintMaxIds * 4, 0);
        if (!out_on_device || staged) {  // host outputs are complete, the caller's host inputs are read
            MC_HIP(hipStreamSynchronize(s));
            ctx->timer.collect();
        }
    });
}

}  // extern "C"
