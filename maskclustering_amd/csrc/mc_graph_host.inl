// mc_graph_host.inl — scene input, S2–S5 and level-0 nodes: the host side (included by mc_api.hip,
// same translation unit).  mc_scene_set_masks is scene_keep_masks (validation and the frame-skip
// rule), scene_upload and scene_reserve; mc_graph_build is graph_s2_point_lists, graph_s3_masks and
// then either the sharded hand-off (mc_shard_host.inl) or graph_undo_s5_hist and graph_thresholds.
// The frame starts, this rank's rows, the S3 work lists and the histogram replicas are
// mc_graph_plan.hpp's.
namespace {

constexpr size_t kHistTilesLds = 2 * mc::kHistTile * mc::kHistKW * sizeof(unsigned long long);

// Both S4 kernels size their LDS by the frame count (mc_graph_plan.hpp).  A request above the
// device's limit per workgroup is refused here, before any S4 launch, not left to the launch.
void s4_require_lds(const mc_ctx *ctx, int F)
{
    const size_t limit = static_cast<size_t>(std::max(ctx->max_lds, 0));
    MC_REQUIRE(mc::hist_lds_bytes(F, kHistTilesLds) <= limit, MC_ERR_UNSUPPORTED,
               "observer histogram: the LDS for this many frames exceeds the device's limit per workgroup");
    MC_REQUIRE(mc::thresholds_lds_bytes(F, mc::kS4ThrStaticLds) <= limit, MC_ERR_UNSUPPORTED,
               "observer thresholds: the LDS for this many frames exceeds the device's limit per workgroup");
}

// S4 histogram launch: persistent blocks, R lane-indexed LDS replicas (odd stride)
// rng: >= ceil(M / 64) int2 of scratch; the caller has passed s4_require_lds
void launch_hist(hipStream_t s, const unsigned long long *vf, int M, int F, unsigned long long *hist, int2 *rng,
                 int shard_rank = 0, int shard_world = 1)
{
    if (!M || !F) return;
    const int FW = (F + 63) / 64;
    const int nblk = ceil_div(M, mc::kHistTile);
    hipLaunchKernelGGL(mc::k_s4_ranges, grid_for(static_cast<int64_t>(nblk) * 64), dim3(256), 0, s, vf, M, FW, nblk, rng);
    const long long ntiles = static_cast<long long>(nblk) * (nblk + 1) / 2;
    const int HS = mc::hist_stride(F), R = mc::hist_replicas(F);
    const size_t lds = mc::hist_lds_bytes(F, kHistTilesLds);
    const long long grid = std::min<long long>(ntiles, 1024);
    hipLaunchKernelGGL(mc::k_s4_hist, dim3(static_cast<unsigned>(grid)), dim3(256), lds, s, vf, M, FW, F, nblk, ntiles, R,
                       HS, rng, hist, shard_rank, shard_world);
}

// this rank's mask rows [shard.r0, shard.r1) (all rows when not sharded) and their S3 work lists, uploaded
void build_s3_lists(mc_ctx *ctx, const std::vector<int32_t> &frame_start)
{
    SceneState &sc = ctx->scene;
    GraphState &gr = ctx->graph;
    ShardState &sh = ctx->shard;
    hipStream_t s = ctx->stream;
    const mc::RowCut rows = mc::shard_row_cut(sc.h_off.data(), sc.M, sh.rank, sh.world);
    const mc::S3Lists l = mc::s3_work_lists(sc.h_off.data(), rows, sc.F, mc::max_masks_per_frame(frame_start),
                                            {mc::kS3wFrameWords64, mc::kS3wCounters, mc::kS3SmallPts});
    sh.r0 = rows.r0;
    sh.r1 = rows.r1;
    gr.n_s3_small = static_cast<int>(l.small.size());
    gr.n_s3_big = static_cast<int>(l.big.size());
    gr.d_s3_small.reserve((l.small.size() + 1) * sizeof(int));
    gr.d_s3_big.reserve((l.big.size() + 1) * sizeof(int));
    if (!l.small.empty())
        MC_HIP(hipMemcpyAsync(gr.d_s3_small.ptr, l.small.data(), l.small.size() * sizeof(int), hipMemcpyHostToDevice, s));
    if (!l.big.empty())
        MC_HIP(hipMemcpyAsync(gr.d_s3_big.ptr, l.big.data(), l.big.size() * sizeof(int), hipMemcpyHostToDevice, s));
    MC_HIP(hipStreamSynchronize(s));
}

// validation + the frame-skip rule (construction.py:50-51): the masks of frames with points, on the host
void scene_keep_masks(mc_ctx *ctx, int32_t num_frames, int32_t num_masks_in, const int32_t *mask_col,
                      const int32_t *mask_label, const int64_t *mask_off)
{
    SceneState &sc = ctx->scene;
    std::vector<int64_t> frame_pts(std::max(1, num_frames), 0);
    std::vector<int> frame_masks(std::max(1, num_frames), 0);
    for (int g = 0; g < num_masks_in; g++) {
        const int c = mask_col[g];
        MC_REQUIRE(c >= 0 && c < num_frames, MC_ERR_INVALID, "mask_col out of range");
        MC_REQUIRE(g == 0 || mask_col[g - 1] <= c, MC_ERR_INVALID, "mask_col must be non-decreasing");
        MC_REQUIRE(mask_label[g] >= 1 && mask_label[g] <= 65535, MC_ERR_INVALID, "mask label must be in [1, 65535]");
        MC_REQUIRE(mask_off[g + 1] >= mask_off[g], MC_ERR_INVALID, "mask_off must be non-decreasing");
        frame_pts[c] += mask_off[g + 1] - mask_off[g];
        frame_masks[c]++;
        MC_REQUIRE(frame_masks[c] < 2048, MC_ERR_UNSUPPORTED, "more than 2047 masks in a frame");
    }
    std::vector<int> seen(65536, -1);
    for (int g = 0; g < num_masks_in; g++) {
        MC_REQUIRE(seen[mask_label[g]] != mask_col[g], MC_ERR_INVALID, "duplicate mask label within a frame");
        seen[mask_label[g]] = mask_col[g];
    }
    sc.h_col.clear();
    sc.h_label.clear();
    sc.h_in_index.clear();
    sc.h_off.assign(1, 0);
    for (int g = 0; g < num_masks_in; g++) {
        if (frame_pts[mask_col[g]] == 0) continue;  // masks of a skipped frame have no points
        sc.h_in_index.push_back(g);
        sc.h_col.push_back(mask_col[g]);
        sc.h_label.push_back(mask_label[g]);
        sc.h_off.push_back(static_cast<int32_t>(mask_off[g + 1]));
    }
    sc.M = static_cast<int>(sc.h_col.size());
    MC_REQUIRE(sc.M <= 262144, MC_ERR_UNSUPPORTED, "more than 262144 global masks");
}

}  // namespace

extern "C" __global__ void k_validate_pts(const int *pts, int nnz, int64_t P, int *bad)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nnz; i += gridDim.x * 256)
        if (pts[i] < 0 || pts[i] >= P) atomicOr(bad, 1);
}

namespace {

// the kept masks and their points on the device; the point ids checked there (one host sync)
void scene_upload(mc_ctx *ctx, const std::vector<int32_t> &frame_start, const int32_t *mask_pts, int pts_on_device)
{
    SceneState &sc = ctx->scene;
    hipStream_t s = ctx->stream;
    const int M = sc.M, F = sc.F, nnz = sc.nnz;
    sc.d_mask_off.reserve((M + 1) * sizeof(int));
    sc.d_mask_col.reserve((M + 1) * sizeof(int));
    sc.d_mask_label.reserve((M + 1) * sizeof(int));
    sc.d_frame_start.reserve((F + 2) * sizeof(int));
    sc.d_mask_pts.reserve((static_cast<int64_t>(nnz) + 1) * sizeof(int));
    sc.d_valid.reserve(sizeof(int));
    MC_HIP(hipMemcpyAsync(sc.d_mask_off.ptr, sc.h_off.data(), (M + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    if (M) {
        MC_HIP(hipMemcpyAsync(sc.d_mask_col.ptr, sc.h_col.data(), M * sizeof(int), hipMemcpyHostToDevice, s));
        MC_HIP(hipMemcpyAsync(sc.d_mask_label.ptr, sc.h_label.data(), M * sizeof(int), hipMemcpyHostToDevice, s));
    }
    MC_HIP(hipMemcpyAsync(sc.d_frame_start.ptr, frame_start.data(), (F + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    if (nnz)
        MC_HIP(hipMemcpyAsync(sc.d_mask_pts.ptr, mask_pts, nnz * sizeof(int),
                              pts_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    MC_HIP(hipMemsetAsync(sc.d_valid.ptr, 0, sizeof(int), s));
    if (nnz)
        hipLaunchKernelGGL(k_validate_pts, grid_for(nnz), dim3(256), 0, s, sc.d_mask_pts.as<int>(), nnz, sc.P,
                           sc.d_valid.as<int>());
    int bad = 0;
    MC_HIP(hipMemcpyAsync(&bad, sc.d_valid.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
    MC_HIP(hipStreamSynchronize(s));
    MC_REQUIRE(bad == 0, MC_ERR_INVALID, "mask point id out of [0, num_points)");
}

// S2/S3/S4 buffers (allocated once per scene; nothing is allocated while building)
void scene_reserve(mc_ctx *ctx)
{
    SceneState &sc = ctx->scene;
    GraphState &gr = ctx->graph;
    const int64_t P = sc.P;
    const int F = sc.F, FW = sc.FW, M = sc.M;
    const size_t MF = static_cast<size_t>(M) * F, MFW = static_cast<size_t>(M) * FW;
    gr.d_deg.reserve((P + 1) * sizeof(int));
    gr.d_spread.reserve(mc::kSpread * mc::kSpreadStrideI * sizeof(int));
    MC_HIP(hipMemsetAsync(gr.d_deg.ptr, 0, (P + 1) * sizeof(int), ctx->stream));  // kept zero by the S2 scatter
    gr.d_pt_off.reserve((P + 2) * sizeof(int));
    gr.d_pt_list.reserve((static_cast<int64_t>(sc.nnz) + 1) * sizeof(unsigned));
    gr.d_boundary.reserve(P + 1);
    gr.d_pfm.reserve((P * FW + 1) * sizeof(unsigned long long));
    gr.d_scan_tmp.reserve((2 * (P / 4096 + 4) + 16) * sizeof(int));
    gr.d_ctmp.reserve((MF + 1) * sizeof(int));
    gr.d_crow_len.reserve((M + 1) * sizeof(int));
    gr.d_useg.reserve(M + 1);
    gr.d_keep_cnt.reserve((M + 1) * sizeof(int));
    gr.d_node_flag.reserve((M + 1) * sizeof(int));
    gr.d_node_pos.reserve((M + 2) * sizeof(int));
    gr.d_c_off.reserve((M + 2) * sizeof(int));
    gr.d_c_idx.reserve((MF + 1) * sizeof(int));
    gr.d_vf.reserve((MFW + 1) * sizeof(unsigned long long));
    gr.d_hist.reserve((F + 2) * sizeof(unsigned long long));
    gr.d_s4rng.reserve((M / 64 + 2) * sizeof(int2));
    gr.d_thr.reserve(32 * sizeof(float));
    gr.d_isint.reserve(32 * sizeof(int));
    gr.d_node0_g.reserve((M + 1) * sizeof(int));
    gr.d_n0_off.reserve((M + 1) * sizeof(int));
    gr.d_n0_len.reserve((M + 1) * sizeof(int));
    gr.d_n0_ptoff.reserve((M + 1) * sizeof(int));
    gr.d_n0_ptlen.reserve((M + 1) * sizeof(int));
    gr.d_n0_vf.reserve((MFW + 1) * sizeof(unsigned long long));
    gr.d_owner0.reserve((MF + 1) * sizeof(int));
    gr.d_node_of_mask.reserve((M + 1) * sizeof(int));
    ctx->cluster.d_obj_of_mask.reserve((M + 1) * sizeof(int));
}

// ---------------------------------------------------------------------------------------------
// S2–S5
// ---------------------------------------------------------------------------------------------
void graph_s2_point_lists(mc_ctx *ctx)
{
    SceneState &sc = ctx->scene;
    GraphState &gr = ctx->graph;
    hipStream_t s = ctx->stream;
    const int64_t P = sc.P;
    const int M = sc.M, nnz = sc.nnz;
    TimedScope ts(ctx->timer, s, "s2_point_lists");
    hipLaunchKernelGGL(mc::k_s2_degree, grid_for(nnz), dim3(256), 0, s, sc.d_mask_pts.as<int>(), nnz,
                       gr.d_deg.as<int>(), ctx->d_stats.as<int>(), static_cast<int>(ST_COUNT), gr.d_spread.as<int>());
    mc::scan_large(s, gr.d_deg.as<int>(), gr.d_pt_off.as<int>(), static_cast<int>(P), gr.d_scan_tmp.as<int>());
    if (M)
        hipLaunchKernelGGL(mc::k_s2_scatter, dim3(M), dim3(256), 0, s, sc.d_mask_off.as<int>(),
                           sc.d_mask_pts.as<int>(), sc.d_mask_col.as<int>(), sc.d_frame_start.as<int>(),
                           gr.d_pt_off.as<int>(), gr.d_deg.as<int>(), gr.d_pt_list.as<unsigned>());
    if (P)
        hipLaunchKernelGGL(mc::k_s2_points, dim3(ceil_div(P, 256)), dim3(256), 0, s, gr.d_pt_off.as<int>(),
                           gr.d_pt_list.as<unsigned>(), static_cast<int>(P), sc.FW,
                           gr.d_boundary.as<unsigned char>(), gr.d_pfm.as<unsigned long long>(),
                           gr.d_spread.as<int>());
}

// S3 over this rank's rows: the large masks (workgroup per mask) on the side stream, concurrent with
// the wave kernel
void graph_s3_masks(mc_ctx *ctx, const mc_graph_params &p)
{
    SceneState &sc = ctx->scene;
    GraphState &gr = ctx->graph;
    if (!sc.M) return;
    hipStream_t s = ctx->stream;
    TimedScope ts(ctx->timer, s, "s3_masks");
    const bool fork = gr.n_s3_big && gr.n_s3_small;
    auto launch = [&](auto kernel, dim3 grid, dim3 block, hipStream_t st, const DevBuf &list, int n) {
        hipLaunchKernelGGL(kernel, grid, block, 0, st, list.as<int>(), n, sc.d_mask_off.as<int>(),
                           sc.d_mask_pts.as<int>(), gr.d_pt_off.as<int>(), gr.d_pt_list.as<unsigned>(),
                           gr.d_boundary.as<unsigned char>(), gr.d_pfm.as<unsigned long long>(), sc.FW,
                           sc.d_frame_start.as<int>(), sc.d_mask_label.as<int>(), sc.F, p.mask_visible_threshold,
                           p.contained_threshold, p.undersegment_filter_threshold, gr.d_ctmp.as<int>(),
                           gr.d_crow_len.as<int>(), gr.d_useg.as<unsigned char>());
    };
    if (fork) {
        MC_HIP(hipEventRecord(ctx->ev_fork, s));
        MC_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
    }
    if (gr.n_s3_big)
        launch(mc::k_s3_masks<mc::kS3BigW>, grid_for(gr.n_s3_big, 1, 8192), dim3(mc::S3Cfg<mc::kS3BigW>::NT),
               fork ? ctx->side : s, gr.d_s3_big, gr.n_s3_big);
    if (gr.n_s3_small)
        launch(mc::k_s3_masks<1>, grid_for(gr.n_s3_small, 4, 16384), dim3(256), s, gr.d_s3_small, gr.n_s3_small);
    if (fork) {
        MC_HIP(hipEventRecord(ctx->ev_join, ctx->side));
        MC_HIP(hipStreamWaitEvent(s, ctx->ev_join, 0));
    }
}

// S3 undo + S5 + S4 (this rank's tiles of the observer histogram when sharded)
void graph_undo_s5_hist(mc_ctx *ctx)
{
    SceneState &sc = ctx->scene;
    GraphState &gr = ctx->graph;
    hipStream_t s = ctx->stream;
    const int F = sc.F, FW = sc.FW, M = sc.M;
    int *stats = ctx->d_stats.as<int>();
    if (M) {  // S3 undo + S5
        TimedScope ts(ctx->timer, s, "s3_undo_s5");
        hipLaunchKernelGGL(mc::k_s3_undo_count, dim3(ceil_div(std::max(M, F + 1), 256)), dim3(256), 0, s,
                           gr.d_ctmp.as<int>(), gr.d_crow_len.as<int>(), gr.d_useg.as<unsigned char>(), M, F,
                           gr.d_keep_cnt.as<int>(), gr.d_node_flag.as<int>(),
                           gr.d_hist.as<unsigned long long>(), gr.d_spread.as<int>(), stats + ST_NBND);
        mc::scan_device_n(s, gr.d_keep_cnt.as<int>(), gr.d_c_off.as<int>(), nullptr, M, stats + ST_NNZC,
                          gr.d_node_flag.as<int>(), gr.d_node_pos.as<int>(), stats + ST_N0);
        hipLaunchKernelGGL(mc::k_s3_undo_write, dim3(ceil_div(M, 256)), dim3(256), 0, s, gr.d_ctmp.as<int>(),
                           gr.d_crow_len.as<int>(), gr.d_useg.as<unsigned char>(), sc.d_mask_col.as<int>(), M,
                           F, FW, gr.d_c_off.as<int>(), gr.d_c_idx.as<int>(),
                           gr.d_vf.as<unsigned long long>());
        hipLaunchKernelGGL(mc::k_s5_nodes, dim3(ceil_div(M, 256)), dim3(256), 0, s, gr.d_node_pos.as<int>(),
                           gr.d_useg.as<unsigned char>(), gr.d_c_off.as<int>(), sc.d_mask_off.as<int>(),
                           gr.d_vf.as<unsigned long long>(), M, FW, gr.d_node0_g.as<int>(),
                           gr.d_n0_off.as<int>(), gr.d_n0_len.as<int>(), gr.d_n0_ptoff.as<int>(),
                           gr.d_n0_ptlen.as<int>(), gr.d_n0_vf.as<unsigned long long>(),
                           gr.d_owner0.as<int>(), gr.d_node_of_mask.as<int>());
    } else {
        MC_HIP(hipMemsetAsync(gr.d_hist.ptr, 0, (F + 1) * sizeof(unsigned long long), s));
    }
    {  // S4: observer histogram (the thresholds follow in graph_thresholds)
        TimedScope ts(ctx->timer, s, "s4_observer_hist");
        launch_hist(s, gr.d_vf.as<unsigned long long>(), M, F, gr.d_hist.as<unsigned long long>(),
                    gr.d_s4rng.as<int2>(), ctx->shard.rank, ctx->shard.world);
    }
    MC_HIP(hipGetLastError());
}

// S4 thresholds from the (summed) histogram; the graph's masks become the level-0 nodes
void graph_thresholds(mc_ctx *ctx)
{
    SceneState &sc = ctx->scene;
    GraphState &gr = ctx->graph;
    hipStream_t s = ctx->stream;
    const int F = sc.F;
    int *stats = ctx->d_stats.as<int>();
    {
        TimedScope ts(ctx->timer, s, "s4_observer_hist");
        hipLaunchKernelGGL(mc::k_s4_thresholds, dim3(1), dim3(256), mc::thresholds_lds_dynamic(F), s,
                           gr.d_hist.as<unsigned long long>(), F, gr.d_thr.as<float>(), gr.d_isint.as<int>(),
                           stats + ST_NTHR, stats + ST_THR_STATUS);
    }
    MC_HIP(hipGetLastError());
    // level-0 nodes live in the graph's buffers
    gr.n0_pool = gr.d_c_idx.as<int>();
    gr.n0_pts = sc.d_mask_pts.as<int>();
    gr.Mn = sc.M;
    gr.n0_pts_total = sc.nnz;
    gr.nodes_from_graph = true;
    gr.have = true;
    gr.have_nodes = true;
}

}  // namespace

extern "C" {

int mc_scene_set_masks(mc_ctx *ctx, int64_t num_points, int32_t num_frames, int32_t num_masks_in,
                       const int32_t *mask_col, const int32_t *mask_label, const int64_t *mask_off,
                       const int32_t *mask_pts, int pts_on_device)
{
    return guarded(ctx, [&] {
        SceneState &sc = ctx->scene;
        MC_REQUIRE(num_points >= 0 && num_points < (int64_t(1) << 31) - 1, MC_ERR_UNSUPPORTED, "num_points out of range");
        MC_REQUIRE(num_frames >= 0 && num_frames <= 16384, MC_ERR_UNSUPPORTED, "num_frames must be <= 16384");
        MC_REQUIRE(num_masks_in >= 0, MC_ERR_INVALID, "num_masks < 0");
        MC_REQUIRE(num_masks_in == 0 || (mask_col && mask_label && mask_off), MC_ERR_INVALID, "null mask arrays");
        MC_REQUIRE(!mask_off || mask_off[0] == 0, MC_ERR_INVALID, "mask_off[0] != 0");
        const int64_t nnz = num_masks_in ? mask_off[num_masks_in] : 0;
        MC_REQUIRE(nnz < (int64_t(1) << 31) - 1, MC_ERR_UNSUPPORTED, "more than 2^31 mask points");
        MC_REQUIRE(nnz == 0 || mask_pts, MC_ERR_INVALID, "null mask_pts");
        sc.have = ctx->graph.have = ctx->graph.have_nodes = ctx->cluster.have = false;
        sc.P = num_points;
        sc.F = num_frames;
        sc.FW = (num_frames + 63) / 64;
        sc.M_in = num_masks_in;
        scene_keep_masks(ctx, num_frames, num_masks_in, mask_col, mask_label, mask_off);
        sc.nnz = static_cast<int>(nnz);
        const std::vector<int32_t> frame_start = mc::frame_starts(sc.h_col.data(), sc.M, sc.F);
        scene_upload(ctx, frame_start, mask_pts, pts_on_device);
        scene_reserve(ctx);
        build_s3_lists(ctx, frame_start);
        sc.have = true;
    });
}

int mc_graph_build(mc_ctx *ctx, const mc_graph_params *params)
{
    return guarded(ctx, [&] {
        ShardState &sh = ctx->shard;
        MC_REQUIRE(ctx->scene.have, MC_ERR_STATE, "mc_graph_build before mc_scene_set_masks");
        MC_REQUIRE(params, MC_ERR_INVALID, "null params");
        s4_require_lds(ctx, ctx->scene.F);
        ctx->cluster.have = false;
        ctx->graph.have = ctx->graph.have_nodes = false;
        sh.pending = 0;
        sh.params = *params;
        graph_s2_point_lists(ctx);
        graph_s3_masks(ctx, *params);
        if (sharded(ctx)) {  // this rank's S3 rows go to the others first (mc_shard_export/import)
            sh.pending = MC_SHARD_S3;
            sh.s3_words = -1;
            if (sh.comm) shard_drain_native(ctx);  // S3 rows, then the histogram, over RCCL
            return;
        }
        graph_undo_s5_hist(ctx);
        graph_thresholds(ctx);
    });
}

int mc_graph_get_info(mc_ctx *ctx, mc_graph_info *info)
{
    return guarded(ctx, [&] {
        SceneState &sc = ctx->scene;
        MC_REQUIRE(ctx->graph.have && info, MC_ERR_STATE, "no graph");
        sync_stats(ctx);
        const int *h = ctx->h_stats;
        info->num_points = sc.P;
        info->num_frames = sc.F;
        info->num_masks = sc.M;
        info->num_nodes0 = h[ST_N0];
        info->num_undersegment = sc.M - h[ST_N0];
        info->num_contained = h[ST_NNZC];
        info->num_boundary = h[ST_NBND];
        info->num_thresholds = h[ST_NTHR];
        info->threshold_status = h[ST_THR_STATUS];
    });
}

int mc_graph_get_global_masks(mc_ctx *ctx, int32_t *input_index)
{
    return guarded(ctx, [&] {
        SceneState &sc = ctx->scene;
        MC_REQUIRE(sc.have, MC_ERR_STATE, "no scene");
        std::copy(sc.h_in_index.begin(), sc.h_in_index.end(), input_index);
    });
}

int mc_graph_get_boundary(mc_ctx *ctx, uint8_t *flags)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->graph.have, MC_ERR_STATE, "no graph");
        fetch(ctx, flags, ctx->graph.d_boundary.ptr, ctx->scene.P);
    });
}

int mc_graph_get_point_in_mask(mc_ctx *ctx, uint16_t *pim)
{
    return guarded(ctx, [&] {
        SceneState &sc = ctx->scene;
        GraphState &gr = ctx->graph;
        MC_REQUIRE(gr.have, MC_ERR_STATE, "no graph");
        const size_t bytes = static_cast<size_t>(sc.P) * sc.F * sizeof(uint16_t);
        if (!bytes) return;
        DevBuf tmp;
        tmp.reserve(bytes);
        MC_HIP(hipMemsetAsync(tmp.ptr, 0, bytes, ctx->stream));
        hipLaunchKernelGGL(mc::k_s2_dense_pim, dim3(ceil_div(sc.P, 256)), dim3(256), 0, ctx->stream,
                           gr.d_pt_off.as<int>(), gr.d_pt_list.as<unsigned>(), sc.d_mask_label.as<int>(),
                           sc.d_frame_start.as<int>(), static_cast<int>(sc.P), sc.F, tmp.as<unsigned short>());
        fetch(ctx, pim, tmp.ptr, bytes);
    });
}

int mc_graph_get_point_frame_bits(mc_ctx *ctx, uint64_t *bits)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->graph.have, MC_ERR_STATE, "no graph");
        fetch(ctx, bits, ctx->graph.d_pfm.ptr, static_cast<size_t>(ctx->scene.P) * ctx->scene.FW * 8);
    });
}

int mc_graph_get_visible_frame_bits(mc_ctx *ctx, uint64_t *bits)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->graph.have, MC_ERR_STATE, "no graph");
        fetch(ctx, bits, ctx->graph.d_vf.ptr, static_cast<size_t>(ctx->scene.M) * ctx->scene.FW * 8);
    });
}

int mc_graph_get_contained(mc_ctx *ctx, int64_t *row_off, int32_t *col_idx)
{
    return guarded(ctx, [&] {
        SceneState &sc = ctx->scene;
        GraphState &gr = ctx->graph;
        MC_REQUIRE(gr.have, MC_ERR_STATE, "no graph");
        sync_stats(ctx);
        std::vector<int32_t> off(sc.M + 1);
        MC_HIP(hipMemcpyAsync(off.data(), gr.d_c_off.ptr, (sc.M + 1) * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        fetch(ctx, col_idx, gr.d_c_idx.ptr, ctx->h_stats[ST_NNZC] * sizeof(int));
        for (int i = 0; i <= sc.M; i++) row_off[i] = sc.M ? off[i] : 0;
    });
}

int mc_graph_get_undersegment(mc_ctx *ctx, int32_t *ids)
{
    return guarded(ctx, [&] {
        SceneState &sc = ctx->scene;
        MC_REQUIRE(ctx->graph.have, MC_ERR_STATE, "no graph");
        std::vector<uint8_t> u(sc.M);
        fetch(ctx, u.data(), ctx->graph.d_useg.ptr, sc.M);
        int k = 0;
        for (int g = 0; g < sc.M; g++)
            if (u[g]) ids[k++] = g;
    });
}

int mc_graph_get_nodes0(mc_ctx *ctx, int32_t *mask_index)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->graph.have, MC_ERR_STATE, "no graph");
        sync_stats(ctx);
        fetch(ctx, mask_index, ctx->graph.d_node0_g.ptr, ctx->h_stats[ST_N0] * sizeof(int));
    });
}

int mc_graph_get_observer_hist(mc_ctx *ctx, uint64_t *hist)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->graph.have, MC_ERR_STATE, "no graph");
        fetch(ctx, hist, ctx->graph.d_hist.ptr, (ctx->scene.F + 1) * 8);
    });
}

int mc_graph_get_thresholds(mc_ctx *ctx, float *thr, int32_t *is_int, int32_t *n)
{
    return guarded(ctx, [&] {
        GraphState &gr = ctx->graph;
        MC_REQUIRE(gr.have, MC_ERR_STATE, "no graph");
        sync_stats(ctx);
        MC_HIP(hipMemcpyAsync(thr, gr.d_thr.ptr, mc::kMaxThresholds * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        fetch(ctx, is_int, gr.d_isint.ptr, mc::kMaxThresholds * sizeof(int));
        *n = ctx->h_stats[ST_NTHR];
        if (ctx->h_stats[ST_THR_STATUS] != MC_OK)
            throw McError{ctx->h_stats[ST_THR_STATUS], "no positive observer count (np.percentile of an empty array)"};
    });
}

int mc_observer_thresholds(mc_ctx *ctx, int32_t num_rows, int32_t num_frames, const uint64_t *vf_bits, float *thr,
                           int32_t *is_int, int32_t *n)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(num_rows >= 0 && num_frames >= 0 && num_frames <= 16384, MC_ERR_INVALID, "bad sizes");
        MC_REQUIRE(thr && is_int && n && (num_rows == 0 || num_frames == 0 || vf_bits), MC_ERR_INVALID, "null argument");
        s4_require_lds(ctx, num_frames);
        hipStream_t s = ctx->stream;
        const int M = num_rows, F = num_frames, FW = (F + 63) / 64;
        DevBuf vf, hist, dthr, disint, st;
        vf.reserve(static_cast<size_t>(M) * FW * 8 + 8);
        hist.reserve((F + 2) * 8);
        dthr.reserve(32 * 4);
        disint.reserve(32 * 4);
        st.reserve(2 * 4);
        if (M && FW) MC_HIP(hipMemcpyAsync(vf.ptr, vf_bits, static_cast<size_t>(M) * FW * 8, hipMemcpyHostToDevice, s));
        MC_HIP(hipMemsetAsync(hist.ptr, 0, (F + 1) * 8, s));
        DevBuf rng;
        rng.reserve((M / 64 + 2) * sizeof(int2));
        launch_hist(s, vf.as<unsigned long long>(), M, F, hist.as<unsigned long long>(), rng.as<int2>());
        hipLaunchKernelGGL(mc::k_s4_thresholds, dim3(1), dim3(256), mc::thresholds_lds_dynamic(F), s,
                           hist.as<unsigned long long>(), F,
                           dthr.as<float>(), disint.as<int>(), st.as<int>(), st.as<int>() + 1);
        MC_HIP(hipGetLastError());  // a refused launch is this call's error, not an unwritten status
        int hs[2];
        MC_HIP(hipMemcpyAsync(hs, st.ptr, 8, hipMemcpyDeviceToHost, s));
        MC_HIP(hipMemcpyAsync(thr, dthr.ptr, mc::kMaxThresholds * 4, hipMemcpyDeviceToHost, s));
        MC_HIP(hipMemcpyAsync(is_int, disint.ptr, mc::kMaxThresholds * 4, hipMemcpyDeviceToHost, s));
        MC_HIP(hipStreamSynchronize(s));
        *n = hs[0];
        if (hs[1] != MC_OK) throw McError{hs[1], "no positive observer count (np.percentile of an empty array)"};
    });
}

// ---------------------------------------------------------------------------------------------
// arbitrary level-0 nodes
// ---------------------------------------------------------------------------------------------
__global__ void k_nodes_from_csr(int n, const int64_t *c_off, const int64_t *pt_off, int *n_off, int *n_len, int *n_ptoff,
                                 int *n_ptlen, int *owner)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        n_off[i] = static_cast<int>(c_off[i]);
        n_len[i] = static_cast<int>(c_off[i + 1] - c_off[i]);
        n_ptoff[i] = static_cast<int>(pt_off[i]);
        n_ptlen[i] = static_cast<int>(pt_off[i + 1] - pt_off[i]);
        for (int64_t e = c_off[i]; e < c_off[i + 1]; e++) owner[e] = i;
    }
}

int mc_nodes_set(mc_ctx *ctx, int32_t num_nodes, int32_t num_frames, int32_t num_masks, int64_t num_points,
                 const uint64_t *vf_bits, const int64_t *c_off, const int32_t *c_idx, const int64_t *pt_off,
                 const int32_t *pt_idx)
{
    return guarded(ctx, [&] {
        SceneState &sc = ctx->scene;
        GraphState &gr = ctx->graph;
        MC_REQUIRE(num_nodes >= 0 && num_frames >= 0 && num_masks >= 0 && num_points >= 0, MC_ERR_INVALID, "negative size");
        MC_REQUIRE(num_frames <= 16384, MC_ERR_UNSUPPORTED, "num_frames must be <= 16384");
        MC_REQUIRE(num_masks <= 262144, MC_ERR_UNSUPPORTED, "num_masks must be <= 262144");
        MC_REQUIRE(num_nodes == 0 || (vf_bits && c_off && pt_off), MC_ERR_INVALID, "null node arrays");
        const int64_t nc = num_nodes ? c_off[num_nodes] : 0, np = num_nodes ? pt_off[num_nodes] : 0;
        MC_REQUIRE(nc < (int64_t(1) << 31) && np < (int64_t(1) << 31), MC_ERR_UNSUPPORTED, "node arrays too large");
        for (int64_t i = 0; i < nc; i++) MC_REQUIRE(c_idx[i] >= 0 && c_idx[i] < num_masks, MC_ERR_INVALID, "contained id out of range");
        for (int64_t i = 0; i < np; i++) MC_REQUIRE(pt_idx[i] >= 0 && pt_idx[i] < num_points, MC_ERR_INVALID, "point id out of range");
        for (int i = 0; i < num_nodes; i++)
            for (int64_t k = c_off[i] + 1; k < c_off[i + 1]; k++)
                MC_REQUIRE(c_idx[k - 1] < c_idx[k], MC_ERR_INVALID, "contained ids must be ascending and unique per node");
        hipStream_t s = ctx->stream;
        gr.have = false;
        ctx->cluster.have = false;
        gr.nodes_from_graph = false;
        sc.F = num_frames;
        sc.FW = (num_frames + 63) / 64;
        sc.P = num_points;
        gr.Mn = num_masks;
        gr.N0 = num_nodes;
        gr.nnzC0 = nc;
        gr.n0_pts_total = np;
        const int n = num_nodes, FW = sc.FW;
        gr.d_n0_off.reserve((n + 1) * sizeof(int));
        gr.d_n0_len.reserve((n + 1) * sizeof(int));
        gr.d_n0_ptoff.reserve((n + 1) * sizeof(int));
        gr.d_n0_ptlen.reserve((n + 1) * sizeof(int));
        gr.d_n0_vf.reserve((static_cast<size_t>(n) * FW + 1) * 8);
        gr.d_user_cidx.reserve((nc + 1) * sizeof(int));
        gr.d_user_pts.reserve((np + 1) * sizeof(int));
        gr.d_owner0.reserve((nc + 1) * sizeof(int));
        DevBuf t1, t2;
        t1.reserve((n + 1) * 8);
        t2.reserve((n + 1) * 8);
        if (n) {
            MC_HIP(hipMemcpyAsync(t1.ptr, c_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
            MC_HIP(hipMemcpyAsync(t2.ptr, pt_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
            if (FW) MC_HIP(hipMemcpyAsync(gr.d_n0_vf.ptr, vf_bits, static_cast<size_t>(n) * FW * 8, hipMemcpyHostToDevice, s));
            if (nc) MC_HIP(hipMemcpyAsync(gr.d_user_cidx.ptr, c_idx, nc * sizeof(int), hipMemcpyHostToDevice, s));
            if (np) MC_HIP(hipMemcpyAsync(gr.d_user_pts.ptr, pt_idx, np * sizeof(int), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_nodes_from_csr, grid_for(n), dim3(256), 0, s, n, t1.as<int64_t>(), t2.as<int64_t>(),
                               gr.d_n0_off.as<int>(), gr.d_n0_len.as<int>(), gr.d_n0_ptoff.as<int>(),
                               gr.d_n0_ptlen.as<int>(), gr.d_owner0.as<int>());
        }
        MC_HIP(hipStreamSynchronize(s));
        gr.n0_pool = gr.d_user_cidx.as<int>();
        gr.n0_pts = gr.d_user_pts.as<int>();
        gr.have_nodes = true;
    });
}

}  // extern "C"
