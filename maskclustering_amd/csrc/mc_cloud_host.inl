// mc_cloud_host.inl — host driver of the scene point cloud fusion (mc_cloud_*, mc_scene_use_cloud; kernels:
// mc_cloud_kernels.inl, decisions: mc_cloud_plan.hpp).  Included by mc_api.hip after the projected boxes.
//
// cloud_stage is one voxel_down_sample on the device; mc_cloud_voxel_down runs it once, mc_cloud_fuse_frames
// once per flushed buffer and once over the concatenated results (tasmap/tasmap2mct_format.py:271-282).
// A call works in buffers of its own and swaps the result into the context last, so a refused call
// leaves the earlier result as it was.  The host waits where it sizes an array from a device count
// (a buffer's valid pixels, a stage's voxels, the fold's class lists), after checking that count.

namespace {

struct CloudRun {
    int64_t stages = 0, max_in = 0, max_pop = 0;
};

void cloud_require(int rc, const std::string &why)
{
    if (rc != mc::kCloudAccept) throw McError{rc == mc::kCloudInvalid ? MC_ERR_INVALID : MC_ERR_UNSUPPORTED, why};
}

int64_t cloud_budget(mc_ctx *ctx)
{
    size_t free_b = 0, total_b = 0;
    if (ctx->bp.mem_budget <= 0) MC_HIP(hipMemGetInfo(&free_b, &total_b));
    return mc::cloud_byte_budget(ctx->bp.mem_budget, free_b);
}

template <int kCol>
void cloud_fold(mc_ctx *ctx, int nv, const int *voff, int *list, const double *pts, const void *col, double *out_pts,
                double *out_col, int *ints, int *cls_mid, int *cls_big, int h_ints[4])
{
    hipStream_t s = ctx->stream;
    {
        TimedScope ts(ctx->timer, s, "cloud_fold_small");
        hipLaunchKernelGGL(mc::k_cloud_fold_small<kCol>, dim3(ceil_div(nv, 256)), dim3(256), 0, s, nv, voff, list, pts, col,
                           out_pts, out_col, ints + 2, cls_mid, cls_big);
        MC_HIP(hipGetLastError());
    }
    fetch(ctx, h_ints, ints, 16);  // [1] the largest population, [2], [3] the voxels handed to the block kernels
    if (h_ints[2] > 0) {
        TimedScope ts(ctx->timer, s, "cloud_fold_lds");
        hipLaunchKernelGGL((mc::k_cloud_fold_block<true, kCol, 256>), dim3(h_ints[2]), dim3(256), 0, s, cls_mid, voff, list, pts,
                           col, out_pts, out_col);
        MC_HIP(hipGetLastError());
    }
    if (h_ints[3] > 0) {
        TimedScope ts(ctx->timer, s, "cloud_fold_global");
        hipLaunchKernelGGL((mc::k_cloud_fold_block<false, kCol, 1024>), dim3(h_ints[3]), dim3(1024), 0, s, cls_big, voff, list,
                           pts, col, out_pts, out_col);
        MC_HIP(hipGetLastError());
    }
}

// One voxel_down_sample of n device points (colours: none, bytes or float64, kCol) into out_pts / out_col;
// returns the number of voxels.  extra: bytes the caller holds beside the stage's own (for the budget).
int64_t cloud_stage(mc_ctx *ctx, int64_t n, const double *pts, const void *col, int kcol, double voxel, int64_t extra,
                    int64_t budget, DevBuf &out_pts, DevBuf &out_col, CloudRun &run)
{
    run.stages++;
    run.max_in = std::max(run.max_in, n);
    if (n == 0) return 0;
    std::string why;
    cloud_require(mc::cloud_check_count(n, kcol == mc::kCloudNone ? 0 : (kcol == mc::kCloudU8 ? 3 : 24), extra, budget, &why), why);
    hipStream_t s = ctx->stream;
    const dim3 gn(static_cast<unsigned>((n + 255) / 256));
    DevBuf partial, bounds, ints;
    const int nb = static_cast<int>(std::min<int64_t>(1024, (n + 255) / 256));
    partial.reserve(static_cast<size_t>(nb) * 48);
    bounds.reserve(48);
    ints.reserve(16);  // [0] non-finite flag, [1] largest population, [2], [3] class list lengths
    MC_HIP(hipMemsetAsync(ints.ptr, 0, 16, s));
    {
        TimedScope ts(ctx->timer, s, "cloud_bounds");
        hipLaunchKernelGGL(mc::k_cloud_bounds, dim3(nb), dim3(256), 0, s, pts, n, partial.as<double>(), ints.as<int>());
        hipLaunchKernelGGL(mc::k_cloud_bounds_final, dim3(1), dim3(256), 0, s, partial.as<double>(), nb, bounds.as<double>());
        MC_HIP(hipGetLastError());
    }
    double hb[6];
    int h_ints[4] = {0, 0, 0, 0};
    MC_HIP(hipMemcpyAsync(hb, bounds.ptr, 48, hipMemcpyDeviceToHost, s));
    fetch(ctx, h_ints, ints.ptr, 16);
    cloud_require(mc::cloud_check_extent(hb, hb + 3, !(h_ints[0] & 1), voxel, &why), why);

    const uint64_t T = mc::cloud_table_size(n);
    const int lg = mc::cloud_table_log2(T);
    DevBuf tab, cnt, first, slot_of, flag, vnum, scan_tmp;
    tab.reserve(T * 8);
    cnt.reserve(T * 4);
    first.reserve(T * 4);
    slot_of.reserve(static_cast<size_t>(n) * 4);
    flag.reserve(static_cast<size_t>(n + 1) * 4);
    vnum.reserve(static_cast<size_t>(n + 1) * 4);
    scan_tmp.reserve((static_cast<size_t>(n) / mc::kScanTile + 4) * 8 + 64);
    MC_HIP(hipMemsetAsync(tab.ptr, 0xFF, T * 8, s));
    MC_HIP(hipMemsetAsync(cnt.ptr, 0, T * 4, s));
    MC_HIP(hipMemsetAsync(first.ptr, 0xFF, T * 4, s));
    {
        TimedScope ts(ctx->timer, s, "cloud_hash");
        hipLaunchKernelGGL(mc::k_cloud_insert, gn, dim3(256), 0, s, pts, n, bounds.as<double>(), voxel,
                           tab.as<unsigned long long>(), lg, cnt.as<int>(), first.as<unsigned>(), slot_of.as<unsigned>());
        MC_HIP(hipGetLastError());
    }
    {
        TimedScope ts(ctx->timer, s, "cloud_order");
        hipLaunchKernelGGL(mc::k_cloud_flag, gn, dim3(256), 0, s, n, slot_of.as<unsigned>(), first.as<unsigned>(), flag.as<int>());
        mc::scan_large(s, flag.as<int>(), vnum.as<int>(), static_cast<int>(n), scan_tmp.as<int>());
        MC_HIP(hipGetLastError());
    }
    int nv = 0;
    fetch(ctx, &nv, vnum.as<int>() + n, 4);
    MC_REQUIRE(nv >= 1 && nv <= n, MC_ERR_HIP, "voxel count outside [1, n]");
    tab.release();  // the keys have done their work; the entries' count words are read on
    DevBuf vcnt, voff, cursor, list, cls_mid, cls_big;
    vcnt.reserve(static_cast<size_t>(nv + 1) * 4);
    voff.reserve(static_cast<size_t>(nv + 1) * 4);
    cursor.reserve(static_cast<size_t>(nv) * 4);
    list.reserve(static_cast<size_t>(n) * 4);
    const size_t cls_cap = static_cast<size_t>(n) / (mc::kCloudThreadMax + 1) + 1;  // a listed voxel has more points than that
    cls_mid.reserve(cls_cap * 4);
    cls_big.reserve(cls_cap * 4);
    out_pts.reserve(static_cast<size_t>(nv) * 24);
    if (kcol != mc::kCloudNone) out_col.reserve(static_cast<size_t>(nv) * 24);
    MC_HIP(hipMemsetAsync(cursor.ptr, 0, static_cast<size_t>(nv) * 4, s));
    {
        TimedScope ts(ctx->timer, s, "cloud_order");
        hipLaunchKernelGGL(mc::k_cloud_voxels, gn, dim3(256), 0, s, n, flag.as<int>(), vnum.as<int>(), slot_of.as<unsigned>(),
                           cnt.as<int>(), vcnt.as<int>(), ints.as<int>() + 1);
        MC_HIP(hipGetLastError());
    }
    {
        TimedScope ts(ctx->timer, s, "cloud_lists");
        mc::scan_large(s, vcnt.as<int>(), voff.as<int>(), nv, scan_tmp.as<int>());
        hipLaunchKernelGGL(mc::k_cloud_scatter, gn, dim3(256), 0, s, n, slot_of.as<unsigned>(), cnt.as<int>(), voff.as<int>(),
                           cursor.as<int>(), list.as<int>());
        MC_HIP(hipGetLastError());
    }
    double *op = out_pts.as<double>(), *oc = kcol != mc::kCloudNone ? out_col.as<double>() : nullptr;
    if (kcol == mc::kCloudNone)
        cloud_fold<mc::kCloudNone>(ctx, nv, voff.as<int>(), list.as<int>(), pts, col, op, oc, ints.as<int>(), cls_mid.as<int>(),
                                   cls_big.as<int>(), h_ints);
    else if (kcol == mc::kCloudU8)
        cloud_fold<mc::kCloudU8>(ctx, nv, voff.as<int>(), list.as<int>(), pts, col, op, oc, ints.as<int>(), cls_mid.as<int>(),
                                 cls_big.as<int>(), h_ints);
    else
        cloud_fold<mc::kCloudF64>(ctx, nv, voff.as<int>(), list.as<int>(), pts, col, op, oc, ints.as<int>(), cls_mid.as<int>(),
                                  cls_big.as<int>(), h_ints);
    run.max_pop = std::max<int64_t>(run.max_pop, h_ints[1]);
    MC_HIP(hipStreamSynchronize(s));  // the stage's arrays are freed on return
    ctx->timer.collect();
    return nv;
}

void cloud_commit(mc_ctx *ctx, int64_t n, DevBuf &pts, DevBuf &col, bool have_col, const CloudRun &run)
{
    CloudState &c = ctx->cloud;
    c.pts.swap(pts);
    c.col.swap(col);
    c.n = n;
    c.have = true;
    c.have_col = have_col;
    c.stages = run.stages, c.max_in = run.max_in, c.max_pop = run.max_pop;
}

bool cloud_all_finite(const double *a, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(a[i])) return false;
    return true;
}

}  // namespace

extern "C" {

void mc_cloud_params_default(mc_cloud_params *p)
{
    if (!p) return;
    p->voxel_size = 0.005;
    p->depth_trunc = 20.0;
    p->buffer_frames = 10;
}

int mc_cloud_voxel_down(mc_ctx *ctx, int64_t num_points, const double *points, const double *colors, double voxel_size,
                        int on_device)
{
    return guarded(ctx, [&] {
        const int64_t n = num_points;
        MC_REQUIRE(n >= 0, MC_ERR_INVALID, "negative size");
        MC_REQUIRE(voxel_size > 0.0 && std::isfinite(voxel_size), MC_ERR_INVALID, "voxel_size must be positive and finite");
        MC_REQUIRE(n == 0 || points, MC_ERR_INVALID, "null points");
        const int kcol = colors ? mc::kCloudF64 : mc::kCloudNone;
        const int64_t budget = cloud_budget(ctx);
        std::string why;
        cloud_require(mc::cloud_check_count(n, colors ? 24 : 0, 0, budget, &why), why);
        hipStream_t s = ctx->stream;
        DevBuf in_pts, in_col, out_pts, out_col;
        const double *dp = points, *dc = colors;
        if (!on_device && n) {
            in_pts.reserve(static_cast<size_t>(n) * 24);
            MC_HIP(hipMemcpyAsync(in_pts.ptr, points, static_cast<size_t>(n) * 24, hipMemcpyHostToDevice, s));
            dp = in_pts.as<double>();
            if (colors) {
                in_col.reserve(static_cast<size_t>(n) * 24);
                MC_HIP(hipMemcpyAsync(in_col.ptr, colors, static_cast<size_t>(n) * 24, hipMemcpyHostToDevice, s));
                dc = in_col.as<double>();
            }
        }
        CloudRun run;
        const int64_t nv = cloud_stage(ctx, n, dp, dc, kcol, voxel_size, 0, budget, out_pts, out_col, run);
        MC_HIP(hipStreamSynchronize(s));
        cloud_commit(ctx, nv, out_pts, out_col, colors != nullptr, run);
    });
}

int mc_cloud_fuse_frames(mc_ctx *ctx, int32_t num_frames, int32_t height, int32_t width, const float *depth,
                         const uint8_t *rgb, const double *intrinsics, const double *poses, int on_device,
                         const mc_cloud_params *params)
{
    return guarded(ctx, [&] {
        mc_cloud_params prm;
        mc_cloud_params_default(&prm);
        if (params) prm = *params;
        const int F = num_frames, H = height, W = width;
        MC_REQUIRE(F >= 0 && H >= 0 && W >= 0, MC_ERR_INVALID, "negative size");
        MC_REQUIRE(prm.voxel_size > 0.0 && std::isfinite(prm.voxel_size), MC_ERR_INVALID,
                   "voxel_size must be positive and finite");
        MC_REQUIRE(prm.buffer_frames >= 1, MC_ERR_INVALID, "buffer_frames must be at least 1");
        MC_REQUIRE(!std::isnan(prm.depth_trunc), MC_ERR_INVALID, "depth_trunc is NaN");
        const int64_t hw = static_cast<int64_t>(H) * W;
        MC_REQUIRE(F == 0 || (intrinsics && poses && (hw == 0 || (depth && rgb))), MC_ERR_INVALID, "null argument");
        hipStream_t s = ctx->stream;
        // the cameras on the host (checked there) and on the device
        std::vector<double> hK(static_cast<size_t>(F) * 4), hT(static_cast<size_t>(F) * 16);
        if (F) {
            if (on_device) {
                MC_HIP(hipMemcpyAsync(hK.data(), intrinsics, hK.size() * 8, hipMemcpyDeviceToHost, s));
                fetch(ctx, hT.data(), poses, hT.size() * 8);
            } else {
                memcpy(hK.data(), intrinsics, hK.size() * 8);
                memcpy(hT.data(), poses, hT.size() * 8);
            }
        }
        MC_REQUIRE(cloud_all_finite(hK.data(), hK.size()) && cloud_all_finite(hT.data(), hT.size()), MC_ERR_INVALID,
                   "a non-finite intrinsic or pose entry");
        const auto sched = mc::cloud_flush_schedule(F, prm.buffer_frames);
        for (const auto &st : sched)
            MC_REQUIRE((st.second - st.first) * hw < mc::kCloudMaxPoints, MC_ERR_UNSUPPORTED,
                       "a buffer of 2^31 pixels or more: lower buffer_frames");
        const int64_t budget = cloud_budget(ctx);
        DevBuf dK, dT, aff, rk;
        const double *cK = intrinsics, *cT = poses;
        if (F) {
            if (!on_device) {
                dK.reserve(hK.size() * 8);
                dT.reserve(hT.size() * 8);
                MC_HIP(hipMemcpyAsync(dK.ptr, hK.data(), hK.size() * 8, hipMemcpyHostToDevice, s));
                MC_HIP(hipMemcpyAsync(dT.ptr, hT.data(), hT.size() * 8, hipMemcpyHostToDevice, s));
                cK = dK.as<double>(), cT = dT.as<double>();
            }
            aff.reserve(static_cast<size_t>(F) * 4);
            rk.reserve(static_cast<size_t>(F) * 16);
            hipLaunchKernelGGL(mc::k_cloud_frame_prep, dim3(ceil_div(F, 64)), dim3(64), 0, s, F, cK, cT, prm.depth_trunc,
                               aff.as<int>(), rk.as<double>());
            MC_HIP(hipGetLastError());
        }
        CloudRun run;
        std::vector<std::unique_ptr<DevBuf>> part_pts, part_col;
        std::vector<int64_t> part_n;
        int64_t total = 0;
        DevBuf in_depth, in_rgb, tile_cnt, tile_off, scan_tmp, pts, col;
        for (const auto &st : sched) {
            const int f0 = st.first, nf = st.second - st.first;
            const int64_t px = nf * hw;
            const int tiles = ceil_div(px, mc::kCloudTilePx);
            const int64_t held = total * 48 + (on_device ? 8ll * (tiles + 2) : mc::cloud_frame_bytes(nf, H, W));
            int n = 0;
            if (px) {
                MC_REQUIRE(held <= budget, MC_ERR_UNSUPPORTED,
                           "a buffer's frames need " + std::to_string(held) + " bytes, the budget is " + std::to_string(budget));
                const float *dd = depth + f0 * hw;
                const uint8_t *dr = rgb + 3 * f0 * hw;
                if (!on_device) {
                    in_depth.reserve(static_cast<size_t>(px) * 4);
                    in_rgb.reserve(static_cast<size_t>(px) * 3);
                    MC_HIP(hipMemcpyAsync(in_depth.ptr, dd, static_cast<size_t>(px) * 4, hipMemcpyHostToDevice, s));
                    MC_HIP(hipMemcpyAsync(in_rgb.ptr, dr, static_cast<size_t>(px) * 3, hipMemcpyHostToDevice, s));
                    dd = in_depth.as<float>(), dr = in_rgb.as<uint8_t>();
                }
                tile_cnt.reserve(static_cast<size_t>(tiles + 1) * 4);
                tile_off.reserve(static_cast<size_t>(tiles + 1) * 4);
                scan_tmp.reserve((static_cast<size_t>(tiles) / mc::kScanTile + 4) * 8 + 64);
                {
                    TimedScope ts(ctx->timer, s, "cloud_input");
                    hipLaunchKernelGGL(mc::k_cloud_count, dim3(tiles), dim3(256), 0, s, dd, px, prm.depth_trunc, tile_cnt.as<int>());
                    mc::scan_large(s, tile_cnt.as<int>(), tile_off.as<int>(), tiles, scan_tmp.as<int>());
                    MC_HIP(hipGetLastError());
                }
                fetch(ctx, &n, tile_off.as<int>() + tiles, 4);
                MC_REQUIRE(n >= 0 && n <= px, MC_ERR_HIP, "valid pixel count outside [0, pixels]");
                if (n) {
                    std::string why;
                    cloud_require(mc::cloud_check_count(n, 3, held, budget, &why), why);
                    pts.reserve(static_cast<size_t>(n) * 24);
                    col.reserve(static_cast<size_t>(n) * 3);
                    TimedScope ts(ctx->timer, s, "cloud_input");
                    hipLaunchKernelGGL(mc::k_cloud_compact, dim3(tiles), dim3(256), 0, s, dd, dr, px, H, W, cK + 4 * f0, cT + 16 * f0,
                                       aff.as<int>() + f0, rk.as<double>() + 2 * f0, prm.depth_trunc, tile_off.as<int>(),
                                       pts.as<double>(), col.as<unsigned char>());
                    MC_HIP(hipGetLastError());
                }
            }
            part_pts.emplace_back(new DevBuf());
            part_col.emplace_back(new DevBuf());
            const int64_t nv = cloud_stage(ctx, n, pts.as<double>(), col.ptr, mc::kCloudU8, prm.voxel_size, held, budget,
                                           *part_pts.back(), *part_col.back(), run);
            part_n.push_back(nv);
            total += nv;
        }
        MC_HIP(hipStreamSynchronize(s));
        in_depth.release(), in_rgb.release(), pts.release(), col.release();
        // `full`: the buffers' results in order, then the last voxel_down_sample over them
        std::string why;
        if (total) cloud_require(mc::cloud_check_count(total, 24, total * 48, budget, &why), why);
        DevBuf full_pts, full_col, res_pts, res_col;
        full_pts.reserve(static_cast<size_t>(total) * 24);
        full_col.reserve(static_cast<size_t>(total) * 24);
        int64_t at = 0;
        for (size_t k = 0; k < part_n.size(); k++) {
            if (!part_n[k]) continue;
            MC_HIP(hipMemcpyAsync(full_pts.as<double>() + 3 * at, part_pts[k]->ptr, static_cast<size_t>(part_n[k]) * 24,
                                  hipMemcpyDeviceToDevice, s));
            MC_HIP(hipMemcpyAsync(full_col.as<double>() + 3 * at, part_col[k]->ptr, static_cast<size_t>(part_n[k]) * 24,
                                  hipMemcpyDeviceToDevice, s));
            at += part_n[k];
        }
        MC_HIP(hipStreamSynchronize(s));
        part_pts.clear(), part_col.clear();
        const int64_t nv = cloud_stage(ctx, total, full_pts.as<double>(), full_col.ptr, mc::kCloudF64, prm.voxel_size, 0, budget,
                                       res_pts, res_col, run);
        MC_HIP(hipStreamSynchronize(s));
        cloud_commit(ctx, nv, res_pts, res_col, true, run);
    });
}

int mc_cloud_info(mc_ctx *ctx, int64_t *out5)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(out5, MC_ERR_INVALID, "null output");
        const CloudState &c = ctx->cloud;
        MC_REQUIRE(c.have, MC_ERR_STATE, "no scene cloud: call mc_cloud_fuse_frames or mc_cloud_voxel_down");
        out5[0] = c.n;
        out5[1] = c.stages;
        out5[2] = c.max_in;
        out5[3] = c.max_pop;
        out5[4] = static_cast<int64_t>(c.pts.bytes + c.col.bytes);
    });
}

int mc_cloud_get(mc_ctx *ctx, double *points, double *colors, int on_device)
{
    return guarded(ctx, [&] {
        const CloudState &c = ctx->cloud;
        MC_REQUIRE(c.have, MC_ERR_STATE, "no scene cloud: call mc_cloud_fuse_frames or mc_cloud_voxel_down");
        MC_REQUIRE(!colors || c.have_col, MC_ERR_STATE, "the scene cloud was made without colours");
        hipStream_t s = ctx->stream;
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        const size_t bytes = static_cast<size_t>(c.n) * 24;
        if (points && bytes) MC_HIP(hipMemcpyAsync(points, c.pts.ptr, bytes, kind, s));
        if (colors && bytes) MC_HIP(hipMemcpyAsync(colors, c.col.ptr, bytes, kind, s));
        MC_HIP(hipStreamSynchronize(s));
    });
}

int mc_scene_use_cloud(mc_ctx *ctx)
{
    return guarded(ctx, [&] {
        const CloudState &c = ctx->cloud;
        MC_REQUIRE(c.have, MC_ERR_STATE, "no scene cloud: call mc_cloud_fuse_frames or mc_cloud_voxel_down");
        MC_REQUIRE(c.n < (int64_t(1) << 31) - 1, MC_ERR_UNSUPPORTED, "num_points out of range");
        hipStream_t s = ctx->stream;
        BpState &bp = ctx->bp;
        bp.P = c.n;
        bp.scene.reserve(static_cast<size_t>(c.n + 1) * 12);
        if (c.n) {
            hipLaunchKernelGGL(mc::k_cloud_to_f32, dim3(static_cast<unsigned>((3 * c.n + 255) / 256)), dim3(256), 0, s, 3 * c.n,
                               c.pts.as<double>(), bp.scene.as<float>());
            MC_HIP(hipGetLastError());
        }
        bp.have_points = true;
        bp.have_result = false;
        bp.grid_radius = -1.f;  // the grid is built by the next mc_backproject
        MC_HIP(hipStreamSynchronize(s));
    });
}

}  // extern "C"
