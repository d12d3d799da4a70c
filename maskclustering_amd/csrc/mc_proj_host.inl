// mc_proj_host.inl — host driver of the projected boxes (mc_proj_*; kernels: mc_proj_kernels.inl,
// arithmetic: mc_proj_plan.hpp).  Included by mc_api.hip after the post-processing driver, whose
// export arrays mc_proj_top_views reads.
//
// Requests reach k_proj_accum in groups: one object and up to kProjMaxTop of its frames, so that the
// object's point ids and coordinates are gathered once per group.  mc_proj_top_views' groups are
// the final objects themselves.  mc_proj_boxes groups host requests here, by object in order of
// first use; device requests are not grouped (a group per request): grouping them takes a sort and
// a read-back per call, more than the repeated gathers cost at the request counts of a scene.

namespace {

void proj_check_camera(int32_t num_frames, int32_t width, int32_t height)
{
    MC_REQUIRE(num_frames >= 0, MC_ERR_INVALID, "negative size");
    MC_REQUIRE(width >= 1 && width <= mc::kProjMaxSide && height >= 1 && height <= mc::kProjMaxSide, MC_ERR_INVALID,
               "width or height outside [1, 2^30]");
}

// the points of the call on the device: the caller's (uploaded when on the host), or the scene's
// float32 points widened exactly
const double *proj_points(mc_ctx *ctx, int64_t P, const double *points, int on_device)
{
    ProjState &q = ctx->proj;
    hipStream_t s = ctx->stream;
    if (points && on_device) return points;
    q.pts.reserve(static_cast<size_t>(P) * 24 + 8);
    if (points) {
        if (P) MC_HIP(hipMemcpyAsync(q.pts.ptr, points, static_cast<size_t>(P) * 24, hipMemcpyHostToDevice, s));
    } else if (P) {
        hipLaunchKernelGGL(mc::k_pp_widen, grid_for(3 * P), dim3(256), 0, s, ctx->bp.scene.as<float>(), 3 * P, q.pts.as<double>());
    }
    return q.pts.as<double>();
}

// intrinsics [F, 4] and world_to_cam [F, 16] on the device
void proj_camera(mc_ctx *ctx, int F, const double *intr, const double *w2c, int on_device, const double *&dintr,
                 const double *&dw2c)
{
    dintr = intr, dw2c = w2c;
    if (on_device) return;
    ProjState &q = ctx->proj;
    pp_upload(ctx->stream, q.intr, intr, static_cast<size_t>(F) * 32);
    pp_upload(ctx->stream, q.w2c, w2c, static_cast<size_t>(F) * 128);
    dintr = q.intr.as<double>(), dw2c = q.w2c.as<double>();
}

// parts of the object with the most points: as many workgroups as it has turns, 64 at most
int proj_parts(int64_t max_points)
{
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(64, (max_points + mc::kProjChunk - 1) / mc::kProjChunk)));
}

// init, accumulate, finish for n requests in ngroups groups (device arrays; see k_proj_accum)
void proj_launch(mc_ctx *ctx, int n, int ngroups, int parts, const int *gobj, const int *goff, int stride, const int *rframe,
                 const int *rout, const int64_t *opoff, const int *opts, const double *pts, const double *intr,
                 const double *w2c, int width, int height, const int *pad, int *boxes, int *status, int *inside)
{
    ProjState &q = ctx->proj;
    hipStream_t s = ctx->stream;
    q.acc.reserve(static_cast<size_t>(n) * mc::kProjAccWords * 4);
    TimedScope ts(ctx->timer, s, "proj_boxes");
    hipLaunchKernelGGL(mc::k_proj_init, grid_for(n), dim3(256), 0, s, n, q.acc.as<int>());
    hipLaunchKernelGGL(mc::k_proj_accum, dim3(ngroups, parts), dim3(256), 0, s, gobj, goff, stride, rframe, rout, opoff, opts, pts,
                       intr, w2c, width, height, q.acc.as<int>());
    hipLaunchKernelGGL(mc::k_proj_finish, grid_for(n), dim3(256), 0, s, n, q.acc.as<int>(), pad, boxes, status, inside);
    MC_HIP(hipGetLastError());
}

}  // namespace

extern "C" {

int mc_proj_boxes(mc_ctx *ctx, int64_t num_points, const double *points, int32_t num_objects, const int64_t *obj_pt_off,
                  const int32_t *obj_pts, int32_t num_frames, const double *intrinsics, const double *world_to_cam,
                  int32_t width, int32_t height, int32_t num_requests, const int32_t *req_object, const int32_t *req_frame,
                  int on_device, int32_t *boxes, int32_t *status, int32_t *inside, int out_on_device)
{
    return guarded(ctx, [&] {
        const int64_t P = num_points;
        const int K = num_objects, F = num_frames, n = num_requests;
        MC_REQUIRE(P >= 0 && P < (1ll << 31) && K >= 0 && n >= 0 && n <= (1 << 20), MC_ERR_INVALID, "bad sizes");
        proj_check_camera(F, width, height);
        MC_REQUIRE(obj_pt_off && (F == 0 || (intrinsics && world_to_cam)) && (n == 0 || (req_object && req_frame && boxes && status)),
                   MC_ERR_INVALID, "null argument");
        MC_REQUIRE(points || (ctx->bp.have_points && ctx->bp.P == P), MC_ERR_STATE,
                   "no points: pass points or call mc_scene_set_points with num_points points");
        ProjState &q = ctx->proj;
        hipStream_t s = ctx->stream;
        const int64_t *doff = obj_pt_off;
        const int *dpts = obj_pts, *gobj = nullptr, *goff = nullptr, *rframe = nullptr, *rout = nullptr;
        int ngroups = 0, parts = 1;
        if (!on_device) {
            // every check first; then the requests grouped by object, kProjMaxTop to a group
            MC_REQUIRE(obj_pt_off[0] == 0, MC_ERR_INVALID, "obj_pt_off[0] != 0");
            for (int k = 0; k < K; k++) MC_REQUIRE(obj_pt_off[k + 1] >= obj_pt_off[k], MC_ERR_INVALID, "obj_pt_off not ascending");
            const int64_t np = obj_pt_off[K];
            MC_REQUIRE(np < (1ll << 31), MC_ERR_UNSUPPORTED, "more than 2^31 object points");
            MC_REQUIRE(np == 0 || obj_pts, MC_ERR_INVALID, "null argument");
            for (int64_t i = 0; i < np; i++) MC_REQUIRE(obj_pts[i] >= 0 && obj_pts[i] < P, MC_ERR_INVALID, "point id out of range");
            for (int j = 0; j < n; j++)
                MC_REQUIRE(req_object[j] >= 0 && req_object[j] < K && req_frame[j] >= 0 && req_frame[j] < F, MC_ERR_INVALID,
                           "request object or frame index out of range");
            if (!n) return;
            std::vector<int32_t> head(K, -1), next(n, -1), tail(K, -1), first;  // per object its requests, in order
            for (int j = 0; j < n; j++) {
                const int o = req_object[j];
                if (head[o] < 0) head[o] = j, first.push_back(o);
                else next[tail[o]] = j;
                tail[o] = j;
            }
            q.h_gobj.clear(), q.h_goff.assign(1, 0), q.h_rframe.clear(), q.h_rout.clear();
            int64_t mx = 0;
            for (int o : first) {
                mx = std::max(mx, obj_pt_off[o + 1] - obj_pt_off[o]);
                int in_group = 0;
                for (int j = head[o]; j >= 0; j = next[j]) {
                    if (in_group == mc::kProjMaxTop) q.h_gobj.push_back(o), q.h_goff.push_back(static_cast<int32_t>(q.h_rout.size())), in_group = 0;
                    q.h_rframe.push_back(req_frame[j]);
                    q.h_rout.push_back(j);
                    in_group++;
                }
                q.h_gobj.push_back(o), q.h_goff.push_back(static_cast<int32_t>(q.h_rout.size()));
            }
            ngroups = static_cast<int>(q.h_gobj.size());
            parts = proj_parts(mx);
            pp_upload(s, q.opoff, obj_pt_off, static_cast<size_t>(K + 1) * 8);
            pp_upload(s, q.opts, obj_pts, static_cast<size_t>(np) * 4);
            pp_upload(s, q.gobj, q.h_gobj.data(), static_cast<size_t>(ngroups) * 4);
            pp_upload(s, q.goff, q.h_goff.data(), static_cast<size_t>(ngroups + 1) * 4);
            pp_upload(s, q.rframe, q.h_rframe.data(), static_cast<size_t>(n) * 4);
            pp_upload(s, q.rout, q.h_rout.data(), static_cast<size_t>(n) * 4);
            doff = q.opoff.as<int64_t>(), dpts = q.opts.as<int>();
            gobj = q.gobj.as<int>(), goff = q.goff.as<int>(), rframe = q.rframe.as<int>(), rout = q.rout.as<int>();
        } else {
            // the same checks as a kernel behind one flag word; the host reads the flag and the largest object
            int64_t np = 0;
            MC_HIP(hipMemcpyAsync(&np, obj_pt_off + K, 8, hipMemcpyDeviceToHost, s));
            MC_HIP(hipStreamSynchronize(s));
            MC_REQUIRE(np >= 0, MC_ERR_INVALID, "obj_pt_off not ascending");
            MC_REQUIRE(np < (1ll << 31), MC_ERR_UNSUPPORTED, "more than 2^31 object points");
            MC_REQUIRE(np == 0 || obj_pts, MC_ERR_INVALID, "null argument");
            q.flag.reserve(8);
            MC_HIP(hipMemsetAsync(q.flag.ptr, 0, 8, s));
            hipLaunchKernelGGL(mc::k_proj_validate, grid_for(std::max<int64_t>(std::max<int64_t>(np, K + 1), n)), dim3(256), 0, s, P,
                               K, obj_pt_off, np, obj_pts, F, n, req_object, req_frame, q.flag.as<int>());
            MC_HIP(hipGetLastError());
            int h_flag[2] = {0, 0};
            fetch(ctx, h_flag, q.flag.ptr, 8);
            MC_REQUIRE(!(h_flag[0] & mc::kProjBadOffsets), MC_ERR_INVALID, "obj_pt_off must rise from 0");
            MC_REQUIRE(!(h_flag[0] & mc::kProjBadIndex), MC_ERR_INVALID, "a point id, object or frame index is out of range");
            if (!n) return;
            ngroups = n, parts = proj_parts(h_flag[1]);
            gobj = req_object, rframe = req_frame;  // a group per request, its accumulator the request's own
        }
        const double *dp = proj_points(ctx, P, points, on_device), *dintr, *dw2c;
        proj_camera(ctx, F, intrinsics, world_to_cam, on_device, dintr, dw2c);
        int *dbox = boxes, *dstat = status, *dins = inside;
        if (!out_on_device) {
            q.out_boxes.reserve(static_cast<size_t>(n) * 16);
            q.out_status.reserve(static_cast<size_t>(n) * 4);
            q.out_inside.reserve(static_cast<size_t>(n) * 4);
            dbox = q.out_boxes.as<int>(), dstat = q.out_status.as<int>(), dins = inside ? q.out_inside.as<int>() : nullptr;
        }
        proj_launch(ctx, n, ngroups, parts, gobj, goff, 1, rframe, rout, doff, dpts, dp, dintr, dw2c, width, height, nullptr,
                    dbox, dstat, dins);
        if (!out_on_device) {
            MC_HIP(hipMemcpyAsync(boxes, dbox, static_cast<size_t>(n) * 16, hipMemcpyDeviceToHost, s));
            if (inside) MC_HIP(hipMemcpyAsync(inside, dins, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, s));
            fetch(ctx, status, dstat, static_cast<size_t>(n) * 4);
            ctx->timer.collect();
        } else if (!on_device) {
            MC_HIP(hipStreamSynchronize(s));  // the uploads may still read the caller's host arrays
        }
    });
}

int mc_proj_top_views(mc_ctx *ctx, const double *points, int32_t num_frames, const double *intrinsics,
                      const double *world_to_cam, int32_t width, int32_t height, int on_device, int32_t top_k,
                      int32_t *top_pos, int32_t *top_frame, int32_t *boxes, int32_t *status, int32_t *inside,
                      int out_on_device)
{
    return guarded(ctx, [&] {
        PpState &pp = ctx->pp;
        MC_REQUIRE(top_k >= 1 && top_k <= mc::kProjMaxTop, MC_ERR_INVALID, "top_k outside [1, 16]");
        proj_check_camera(num_frames, width, height);
        MC_REQUIRE(pp.have, MC_ERR_STATE, "no post-processing result");
        MC_REQUIRE(num_frames >= pp.F, MC_ERR_INVALID, "fewer frames than the post-processed scene has");
        const int64_t P = pp.P;
        MC_REQUIRE(points || (ctx->bp.have_points && ctx->bp.P == P), MC_ERR_STATE,
                   "no points: pass points or call mc_scene_set_points");
        const int nf = pp.info.num_final, F = num_frames;
        if (!nf) return;
        MC_REQUIRE(intrinsics && world_to_cam && top_pos && top_frame && boxes && status, MC_ERR_INVALID, "null argument");
        MC_REQUIRE(static_cast<int64_t>(nf) * top_k <= (1 << 30), MC_ERR_UNSUPPORTED, "too many requests");
        pp_build_export(ctx);
        ProjState &q = ctx->proj;
        hipStream_t s = ctx->stream;
        const int n = nf * top_k;
        const int64_t nm = pp.omoff[nf];
        int64_t mx = 0;
        for (int f = 0; f < nf; f++) mx = std::max(mx, pp.opoff[f + 1] - pp.opoff[f]);
        const double *dp = proj_points(ctx, P, points, on_device), *dintr, *dw2c;
        proj_camera(ctx, F, intrinsics, world_to_cam, on_device, dintr, dw2c);
        int *dpos = top_pos, *dfr = top_frame, *dbox = boxes, *dstat = status, *dins = inside;
        if (!out_on_device) {
            q.out_pos.reserve(static_cast<size_t>(n) * 4);
            q.out_frame.reserve(static_cast<size_t>(n) * 4);
            q.out_boxes.reserve(static_cast<size_t>(n) * 16);
            q.out_status.reserve(static_cast<size_t>(n) * 4);
            q.out_inside.reserve(static_cast<size_t>(n) * 4);
            dpos = q.out_pos.as<int>(), dfr = q.out_frame.as<int>(), dbox = q.out_boxes.as<int>();
            dstat = q.out_status.as<int>(), dins = inside ? q.out_inside.as<int>() : nullptr;
        }
        q.ocol.reserve(static_cast<size_t>(nm) * 4 + 8);
        {
            TimedScope ts(ctx->timer, s, "proj_select");
            hipLaunchKernelGGL(mc::k_proj_ocol, dim3(std::min(nf, 4096)), dim3(256), 0, s, nf, pp.d_finobj.as<int>(),
                               pp.d_finnode.as<int>(), pp.d_qoff.as<int64_t>(), pp.d_qobj.as<int>(),
                               pp.d_qcol.as<int>(), pp.d_omoff.as<int64_t>(), q.ocol.as<int>());
            hipLaunchKernelGGL(mc::k_proj_top_select, dim3(std::min(ceil_div(nf, 4), 4096)), dim3(256), 0, s, nf, top_k,
                               pp.d_omoff.as<int64_t>(), pp.d_ocov.as<double>(), q.ocol.as<int>(), dpos, dfr);
            MC_HIP(hipGetLastError());
        }
        proj_launch(ctx, n, nf, proj_parts(mx), nullptr, nullptr, top_k, dfr, nullptr, pp.d_opoff.as<int64_t>(),
                    pp.d_opts.as<int>(), dp, dintr, dw2c, width, height, dfr, dbox, dstat, dins);
        if (!out_on_device) {
            MC_HIP(hipMemcpyAsync(top_pos, dpos, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, s));
            MC_HIP(hipMemcpyAsync(top_frame, dfr, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, s));
            MC_HIP(hipMemcpyAsync(boxes, dbox, static_cast<size_t>(n) * 16, hipMemcpyDeviceToHost, s));
            if (inside) MC_HIP(hipMemcpyAsync(inside, dins, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, s));
            fetch(ctx, status, dstat, static_cast<size_t>(n) * 4);
            ctx->timer.collect();
        } else if (!on_device) {
            MC_HIP(hipStreamSynchronize(s));  // the uploads may still read the caller's host arrays
        }
    });
}

}  // extern "C"
