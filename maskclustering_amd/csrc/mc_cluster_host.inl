// mc_cluster_host.inl — S6 iterative clustering and S7 final point sets: the host side (included by
// mc_api.hip, same translation unit).  One mc_cluster_run is s6_reserve, s6_init, s6_level0_columns,
// then s6_levels: per level s6_pairs (or s6_pairs_dense), s6_components and s6_merge, and after the
// last level s7_ranges and s7_points.  A sharded context runs level 0's pairs on its own rows, hands
// the forest to the exchange (mc_shard_host.inl) and enters s6_levels with the pairs done.  The mode
// and the components route are mc_graph_plan.hpp's.
namespace {

S6Level s6_level0(const mc_ctx *ctx)
{
    return {ctx->d_n0_off.as<int>(), ctx->d_n0_len.as<int>(), ctx->n0_pool, ctx->d_owner0.as<int>(),
            ctx->d_n0_vf.as<unsigned long long>()};
}

// the arrays level t's merge writes level t + 1 to: the A and B pools in turn
S6Level s6_level_after(const mc_ctx *ctx, int t)
{
    if (t % 2 == 0)
        return {ctx->d_offA.as<int>(), ctx->d_lenA.as<int>(), ctx->d_poolA.as<int>(), ctx->d_ownA.as<int>(),
                ctx->d_vfA.as<unsigned long long>()};
    return {ctx->d_offB.as<int>(), ctx->d_lenB.as<int>(), ctx->d_poolB.as<int>(), ctx->d_ownB.as<int>(),
            ctx->d_vfB.as<unsigned long long>()};
}

mc::EdgeCap edge_cap(mc_ctx *ctx)
{
    if (ctx->cap_edges <= 0) return mc::EdgeCap{nullptr, nullptr, 0};
    return mc::EdgeCap{ctx->d_cap_buf.as<unsigned long long>(), ctx->d_cap_cnt.as<unsigned long long>(),
                       static_cast<long long>(ctx->cap_edges)};
}

// the S6/S7 buffers for N0 nodes, nnzC0 contained entries and s6_nthr levels
void s6_reserve(mc_ctx *ctx)
{
    hipStream_t s = ctx->stream;
    const int N0 = ctx->N0, FW = ctx->FW, Mn = ctx->Mn, nthr = ctx->s6_nthr;
    const size_t n0 = static_cast<size_t>(std::max(N0, 1));
    const size_t cap = static_cast<size_t>(std::max<int64_t>(ctx->nnzC0, 1));
    ctx->d_parent.reserve(n0 * 4);
    ctx->d_root.reserve(n0 * 4);
    ctx->d_isroot.reserve(n0 * 4);
    ctx->d_rank.reserve((n0 + 1) * 4);
    ctx->d_label.reserve(n0 * 4);
    ctx->d_levels.reserve(std::max<size_t>(1, static_cast<size_t>(nthr)) * n0 * 4);
    const bool fresh_memcnt = ctx->d_memcnt.bytes < n0 * 4;
    ctx->d_memcnt.reserve(n0 * 4);
    if (fresh_memcnt) MC_HIP(hipMemsetAsync(ctx->d_memcnt.ptr, 0, ctx->d_memcnt.bytes, s));  // kept zero by K9
    ctx->d_memoff.reserve((n0 + 1) * 4);
    ctx->d_ublen.reserve(n0 * 4);
    ctx->d_newoff.reserve((n0 + 1) * 4);
    ctx->d_members.reserve(n0 * 4);
    const bool fresh_colcnt = ctx->d_colcnt.bytes < static_cast<size_t>(Mn + 1) * 4;
    ctx->d_colcnt.reserve((Mn + 1) * 4);
    if (fresh_colcnt) MC_HIP(hipMemsetAsync(ctx->d_colcnt.ptr, 0, ctx->d_colcnt.bytes, s));  // kept zero by K3
    ctx->d_coloff.reserve((Mn + 2) * 4);
    ctx->d_collen.reserve((Mn + 1) * 4);
    ctx->d_colnodes.reserve(cap * 4);
    if (!ctx->d_ovf_n.ptr) {
        ctx->d_ovf_n.reserve((1 + mc::kOvfSlots) * 4);  // [0] unused counter (K5 clears it), [1..] slot locks
        MC_HIP(hipMemsetAsync(ctx->d_ovf_n.ptr, 0, (1 + mc::kOvfSlots) * 4, s));  // locks kept zero
    }
    constexpr int kOvfBlocks = mc::kOvfSlots;
    if (ctx->scratch_n0 < N0) {
        ctx->d_scratch.reserve(static_cast<size_t>(kOvfBlocks) * n0 * 4);
        ctx->d_touched.reserve(static_cast<size_t>(kOvfBlocks) * n0 * 4);
        MC_HIP(hipMemsetAsync(ctx->d_scratch.ptr, 0, static_cast<size_t>(kOvfBlocks) * n0 * 4, s));
        ctx->scratch_n0 = N0;
    }
    ctx->d_edges.reserve(static_cast<size_t>(std::max(nthr, 1)) * mc::kSpread * mc::kSpreadStrideL * 8);  // spread slots
    ctx->d_Nlev.reserve((nthr + 2) * 4);
    ctx->d_cap.reserve((nthr + 2) * 4);
    ctx->d_final_label.reserve(n0 * 4);
    ctx->d_poolA.reserve(cap * 4);
    ctx->d_poolB.reserve(cap * 4);
    ctx->d_ownA.reserve(cap * 4);
    ctx->d_ownB.reserve(cap * 4);
    ctx->d_offA.reserve(n0 * 4);
    ctx->d_offB.reserve(n0 * 4);
    ctx->d_lenA.reserve(n0 * 4);
    ctx->d_lenB.reserve(n0 * 4);
    ctx->d_vfA.reserve(n0 * FW * 8 + 8);
    ctx->d_vfB.reserve(n0 * FW * 8 + 8);
    ctx->d_pmin.reserve(n0 * 4);
    ctx->d_pmax.reserve(n0 * 4);
    ctx->d_nwords.reserve(n0 * 4);
    ctx->d_woff.reserve((n0 + 1) * 4);
    ctx->d_ptcnt.reserve(n0 * 4);
    ctx->d_ptoff_out.reserve((n0 + 1) * 4);
    ctx->d_pts_out.reserve((ctx->n0_pts_total + 1) * 4);
}

// level sizes, pool capacities, labels and edge counters at their start; the edge capture emptied
void s6_init(mc_ctx *ctx)
{
    hipStream_t s = ctx->stream;
    const int N0 = ctx->N0, nthr = ctx->s6_nthr;
    int *stats = ctx->d_stats.as<int>();
    hipLaunchKernelGGL(mc::k6_init, grid_for(std::max<int64_t>(N0, nthr)), dim3(256), 0, s, N0,
                       ctx->d_final_label.as<int>(), ctx->nodes_from_graph ? stats + ST_N0 : nullptr, N0,
                       ctx->d_Nlev.as<int>(), ctx->d_cap.as<int>(), ctx->nodes_from_graph ? stats + ST_NNZC : nullptr,
                       static_cast<int>(ctx->nnzC0), ctx->d_edges.as<unsigned long long>(), nthr);
    if (ctx->cap_edges > 0) {
        ctx->d_cap_buf.reserve(static_cast<size_t>(ctx->cap_edges) * 8);
        ctx->d_cap_cnt.reserve(8);
        MC_HIP(hipMemsetAsync(ctx->d_cap_cnt.ptr, 0, 8, s));
    }
}

// level-0 column lists (nodes contained by each mask), for the sparse pairs
void s6_level0_columns(mc_ctx *ctx)
{
    if (ctx->s6_dense_obs || ctx->s6_nthr <= 0) return;
    hipStream_t s = ctx->stream;
    const int N0 = ctx->N0, Mn = ctx->Mn;
    int *Nlev = ctx->d_Nlev.as<int>(), *dcap = ctx->d_cap.as<int>();
    const S6Level l0 = s6_level0(ctx);
    const dim3 gE = grid_for(std::max<int64_t>(N0, ctx->nnzC0)), gC = grid_for(std::max(N0, Mn), 64, 8192);
    TimedScope ts(ctx->timer, s, "s6_columns");
    hipLaunchKernelGGL(mc::k6_colcount, gE, dim3(256), 0, s, Nlev, dcap, l0.pool, l0.own, ctx->d_parent.as<int>(),
                       ctx->d_colcnt.as<int>());
    mc::scan_device_n(s, ctx->d_colcnt.as<int>(), ctx->d_coloff.as<int>(), nullptr, Mn, nullptr);
    hipLaunchKernelGGL(mc::k6_colscatter, gE, dim3(256), 0, s, dcap, l0.pool, l0.own, ctx->d_coloff.as<int>(),
                       ctx->d_colcnt.as<int>(), ctx->d_colnodes.as<int>());
    hipLaunchKernelGGL(mc::k6_colupdate, gC, dim3(64), 0, s, Mn, Nlev, ctx->d_coloff.as<int>(),
                       ctx->d_collen.as<int>(), ctx->d_colnodes.as<int>(), nullptr, ctx->d_parent.as<int>());
}

// level t's sparse pairs over the pair rows of `rank` of `world` (0 of 1: all of them)
void s6_pairs(mc_ctx *ctx, int t, const S6Level &lv, int rank, int world, mc::EdgeCap cap)
{
    hipStream_t s = ctx->stream;
    const int N0 = ctx->N0;
    TimedScope ts(ctx->timer, s, "s6_pairs");
    const mc::OvfWork ow{ctx->d_scratch.as<int>(), ctx->d_touched.as<int>(), N0, ctx->d_ovf_n.as<int>() + 1};
    hipLaunchKernelGGL(mc::k6_pairs, grid_for(N0, mc::kPairWaves, 2048), dim3(256), 0, s, ctx->d_Nlev.as<int>() + t,
                       lv.off, lv.len, lv.pool, ctx->d_coloff.as<int>(), ctx->d_collen.as<int>(),
                       ctx->d_colnodes.as<int>(), lv.vf, ctx->FW, ctx->d_thr.as<float>(), t, ctx->s6_ctf,
                       ctx->d_parent.as<int>(), ctx->d_edges.as<unsigned long long>(), ow, rank, world, cap);
}

// level t's pairs when every pair with enough observers is linked (connect_threshold <= 0)
void s6_pairs_dense(mc_ctx *ctx, int t, const S6Level &lv)
{
    hipStream_t s = ctx->stream;
    const int *dN = ctx->d_Nlev.as<int>() + t;
    TimedScope ts(ctx->timer, s, "s6_pairs");
    hipLaunchKernelGGL(mc::k6_parent_init, grid_for(ctx->N0), dim3(256), 0, s, dN, ctx->d_parent.as<int>());
    hipLaunchKernelGGL(mc::k6_pairs_dense, dim3(4096), dim3(256), 0, s, dN, lv.vf, ctx->FW, ctx->d_thr.as<float>(), t,
                       ctx->d_parent.as<int>(), ctx->d_edges.as<unsigned long long>(), edge_cap(ctx));
}

// connected components of level t's forest: labels, members and row offsets of level t + 1
void s6_components(mc_ctx *ctx, int t, const S6Level &lv)
{
    hipStream_t s = ctx->stream;
    const int N0 = ctx->N0;
    const int *dN = ctx->d_Nlev.as<int>() + t;
    int *dNn = ctx->d_Nlev.as<int>() + t + 1, *dcapn = ctx->d_cap.as<int>() + t + 1;
    int *levels_t = ctx->d_levels.as<int>() + static_cast<size_t>(t) * static_cast<size_t>(std::max(N0, 1));
    const dim3 gN = grid_for(N0);
    TimedScope ts(ctx->timer, s, "s6_components");
    if (mc::s6_components_fused(t, N0)) {  // N_t <= N_1, typically N0 / 8: one workgroup
        hipLaunchKernelGGL(mc::k6_components, dim3(1), dim3(1024), 0, s, dN, dNn, ctx->d_parent.as<int>(),
                           ctx->d_root.as<int>(), ctx->d_rank.as<int>(), lv.len, ctx->d_label.as<int>(), levels_t,
                           ctx->d_memcnt.as<int>(), ctx->d_memoff.as<int>(), ctx->d_ublen.as<int>(),
                           ctx->d_newoff.as<int>(), dcapn, ctx->d_members.as<int>(), ctx->d_ovf_n.as<int>());
        return;
    }
    hipLaunchKernelGGL(mc::k6_compress, gN, dim3(256), 0, s, dN, ctx->d_parent.as<int>(), ctx->d_root.as<int>(),
                       ctx->d_isroot.as<int>(), ctx->d_ublen.as<int>(), ctx->d_ovf_n.as<int>());
    mc::scan_device_n(s, ctx->d_isroot.as<int>(), ctx->d_rank.as<int>(), dN, 0, dNn);
    hipLaunchKernelGGL(mc::k6_relabel, gN, dim3(256), 0, s, dN, ctx->d_root.as<int>(), ctx->d_rank.as<int>(), lv.len,
                       ctx->d_label.as<int>(), levels_t, ctx->d_memcnt.as<int>(), ctx->d_ublen.as<int>());
    mc::scan_device_n(s, ctx->d_memcnt.as<int>(), ctx->d_memoff.as<int>(), dNn, 0, nullptr, ctx->d_ublen.as<int>(),
                      ctx->d_newoff.as<int>(), dcapn);
    hipLaunchKernelGGL(mc::k6_memscatter, gN, dim3(256), 0, s, dN, 0, ctx->d_label.as<int>(), ctx->d_memoff.as<int>(),
                       ctx->d_memcnt.as<int>(), ctx->d_members.as<int>(), nullptr);
}

// level t + 1's nodes from the components' members, + the next level's column lists (nodes
// containing each mask, relabelled)
void s6_merge(mc_ctx *ctx, int t, const S6Level &lv, const S6Level &nx)
{
    hipStream_t s = ctx->stream;
    const int *dNn = ctx->d_Nlev.as<int>() + t + 1;
    const bool cols = !ctx->s6_dense_obs && t + 1 < ctx->s6_nthr;
    TimedScope ts(ctx->timer, s, "s6_merge");
    const mc::ColUpdate cu{ctx->Mn, dNn, ctx->d_coloff.as<int>(), ctx->d_collen.as<int>(), ctx->d_colnodes.as<int>(),
                           cols ? ctx->d_label.as<int>() : nullptr, ctx->d_parent.as<int>(), ctx->N0,
                           ctx->d_label.as<int>(), ctx->d_final_label.as<int>()};
    hipLaunchKernelGGL(mc::k6_merge, grid_for(ctx->N0, 1, 2048), dim3(256), 0, s, dNn, ctx->d_memoff.as<int>(),
                       ctx->d_members.as<int>(), lv.off, lv.len, lv.pool, lv.vf, ctx->FW, ctx->d_newoff.as<int>(), nx.off,
                       nx.len, nx.pool, nx.own, nx.vf, cu);
}

// S7 ranges (node.py:35): every object's point-id range and the words of its range bitmap, from the
// point lists (by_point; ST_OBJOVF tells of a point in more objects than that path holds) or from
// the nodes' point lists; the sizes come to the host
void s7_ranges(mc_ctx *ctx, bool by_point)
{
    hipStream_t s = ctx->stream;
    const int N0 = ctx->N0;
    const int *dK = ctx->d_Nlev.as<int>() + ctx->n_iter;
    int *stats = ctx->d_stats.as<int>();
    const dim3 gN = grid_for(N0);
    {
        TimedScope ts(ctx->timer, s, "s7_points");
        hipLaunchKernelGGL(mc::k7_reset, gN, dim3(256), 0, s, N0, ctx->d_pmin.as<int>(), ctx->d_pmax.as<int>());
        if (by_point) {
            hipLaunchKernelGGL(mc::k7_obj_of_mask, grid_for(ctx->M), dim3(256), 0, s, ctx->M,
                               ctx->d_node_of_mask.as<int>(), ctx->d_final_label.as<int>(),
                               ctx->d_obj_of_mask.as<int>());
            hipLaunchKernelGGL(mc::k7p_points<0>, dim3(ceil_div(ctx->P, 256)), dim3(256), 0, s, static_cast<int>(ctx->P),
                               ctx->d_pt_off.as<int>(), ctx->d_pt_list.as<unsigned>(), ctx->d_frame_start.as<int>(),
                               ctx->d_obj_of_mask.as<int>(), ctx->d_pmin.as<int>(), ctx->d_pmax.as<int>(), nullptr,
                               nullptr, stats + ST_OBJOVF);
        } else {
            hipLaunchKernelGGL(mc::k7_minmax, grid_for(N0, mc::kPairWaves, 2048), dim3(256), 0, s, N0,
                               ctx->d_final_label.as<int>(), ctx->d_n0_ptoff.as<int>(), ctx->d_n0_ptlen.as<int>(),
                               ctx->n0_pts, ctx->d_pmin.as<int>(), ctx->d_pmax.as<int>());
        }
        hipLaunchKernelGGL(mc::k7_words, gN, dim3(256), 0, s, dK, ctx->d_pmin.as<int>(), ctx->d_pmax.as<int>(),
                           ctx->d_nwords.as<int>(), stats + ST_K);
        mc::scan_device_n(s, ctx->d_nwords.as<int>(), ctx->d_woff.as<int>(), dK, 0, stats + ST_WORDS);
    }
    sync_stats(ctx);  // bitmap capacity
    ctx->K = ctx->h_stats[ST_K];
}

// S7 points: the objects' range bitmaps set (by point or by node), counted and extracted
void s7_points(mc_ctx *ctx, bool by_point)
{
    hipStream_t s = ctx->stream;
    const int N0 = ctx->N0;
    const int *dK = ctx->d_Nlev.as<int>() + ctx->n_iter;
    int *stats = ctx->d_stats.as<int>();
    const dim3 gK = grid_for(N0, 1, 2048);
    const size_t words = static_cast<size_t>(std::max(ctx->h_stats[ST_WORDS], 1));
    ctx->d_bm.reserve(words * 8);
    TimedScope ts(ctx->timer, s, "s7_points");
    MC_HIP(hipMemsetAsync(ctx->d_bm.ptr, 0, words * 8, s));
    if (by_point)
        hipLaunchKernelGGL(mc::k7p_points<1>, dim3(ceil_div(ctx->P, 256)), dim3(256), 0, s, static_cast<int>(ctx->P),
                           ctx->d_pt_off.as<int>(), ctx->d_pt_list.as<unsigned>(), ctx->d_frame_start.as<int>(),
                           ctx->d_obj_of_mask.as<int>(), ctx->d_pmin.as<int>(), ctx->d_pmax.as<int>(),
                           ctx->d_woff.as<int>(), ctx->d_bm.as<unsigned long long>(), stats + ST_OBJOVF);
    else
        hipLaunchKernelGGL(mc::k7_setbits, grid_for(N0, mc::kPairWaves, 2048), dim3(256), 0, s, N0,
                           ctx->d_final_label.as<int>(), ctx->d_n0_ptoff.as<int>(), ctx->d_n0_ptlen.as<int>(), ctx->n0_pts,
                           ctx->d_pmin.as<int>(), ctx->d_woff.as<int>(), ctx->d_bm.as<unsigned long long>());
    hipLaunchKernelGGL(mc::k7_count, gK, dim3(256), 0, s, dK, ctx->d_woff.as<int>(), ctx->d_bm.as<unsigned long long>(),
                       ctx->d_ptcnt.as<int>());
    mc::scan_device_n(s, ctx->d_ptcnt.as<int>(), ctx->d_ptoff_out.as<int>(), dK, 0, stats + ST_NPTS);
    hipLaunchKernelGGL(mc::k7_extract, gK, dim3(256), 0, s, dK, ctx->d_woff.as<int>(), ctx->d_bm.as<unsigned long long>(),
                       ctx->d_pmin.as<int>(), ctx->d_ptoff_out.as<int>(), ctx->d_pts_out.as<int>());
}

// the S6 levels (pairs0_done: level 0's pairs ran on every rank's rows and their forests were
// united) and the final objects with their point sets; level t + 1 lives in the ping-pong pools
void s6_levels(mc_ctx *ctx, bool pairs0_done)
{
    S6Level lv = s6_level0(ctx);
    for (int t = 0; t < ctx->s6_nthr; t++) {
        const S6Level nx = s6_level_after(ctx, t);
        if (t > 0 || !pairs0_done) {
            if (ctx->s6_dense_obs) s6_pairs_dense(ctx, t, lv);
            else s6_pairs(ctx, t, lv, 0, 1, edge_cap(ctx));
        }
        s6_components(ctx, t, lv);
        s6_merge(ctx, t, lv, nx);
        lv = nx;
    }
    ctx->fin = lv;
    ctx->n_iter = ctx->s6_nthr;
    const bool point_path = ctx->nodes_from_graph;
    s7_ranges(ctx, point_path);
    const bool use_points = point_path && ctx->h_stats[ST_OBJOVF] == 0;
    if (point_path && !use_points) s7_ranges(ctx, false);  // a point in > 8 objects: redo the ranges per node
    s7_points(ctx, use_points);
    MC_HIP(hipGetLastError());
    MC_HIP(hipMemcpyAsync(ctx->h_stats, ctx->d_stats.ptr, ST_COUNT * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ctx->have_cluster = true;
}

}  // namespace

extern "C" {

int mc_cluster_run(mc_ctx *ctx, const float *thresholds, int32_t n, double connect_threshold)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_nodes, MC_ERR_STATE, "mc_cluster_run before mc_graph_build / mc_nodes_set");
        // (edge capture on a sharded context: iteration 0 evaluates only this rank's pair rows, so its
        // capture holds those rows' edges and the driver gathers them, graph_shard.ShardedGraph.edges;
        // the later iterations run replicated and every rank captures all of their edges)
        hipStream_t s = ctx->stream;
        if (ctx->nodes_from_graph) {
            sync_stats(ctx);  // the one host round trip between S4 and S6 (sizes for the S6 buffers)
            ctx->N0 = ctx->h_stats[ST_N0];
            ctx->nnzC0 = ctx->h_stats[ST_NNZC];
        }
        int nthr;
        if (thresholds) {
            MC_REQUIRE(n >= 0 && n <= 4096, MC_ERR_INVALID, "bad threshold count");
            nthr = n;
            ctx->d_thr.reserve((n + 1) * sizeof(float));
            if (n) MC_HIP(hipMemcpyAsync(ctx->d_thr.ptr, thresholds, n * sizeof(float), hipMemcpyHostToDevice, s));
        } else {
            MC_REQUIRE(ctx->nodes_from_graph, MC_ERR_STATE, "device thresholds need mc_graph_build");
            if (ctx->h_stats[ST_THR_STATUS] != MC_OK)
                throw McError{ctx->h_stats[ST_THR_STATUS], "no positive observer count (np.percentile of an empty array)"};
            nthr = ctx->h_stats[ST_NTHR];
        }
        const int N0 = ctx->N0;
        MC_REQUIRE(!(N0 == 0 && nthr > 0), MC_ERR_NO_NODES, "no nodes to cluster (torch.stack of an empty list)");
        const mc::S6Mode mode = mc::s6_mode(connect_threshold);
        ctx->s6_nthr = nthr;
        ctx->s6_dense_obs = mode.dense_obs;
        ctx->s6_ctf = mode.ctf;
        s6_reserve(ctx);
        s6_init(ctx);
        s6_level0_columns(ctx);
        ctx->have_cluster = false;
        ctx->sh_pending = 0;
        if (nthr > 0 && N0 > 0 && sharded(ctx) && !mode.dense_obs) {
            // iteration 0 (the N0 x N0 pairs) on this rank's rows; the union-find forests of all
            // ranks are united by mc_shard_import(MC_SHARD_FOREST), which runs the rest
            s6_pairs(ctx, 0, s6_level0(ctx), ctx->sh_rank, ctx->sh_world, mc::EdgeCap{nullptr, nullptr, 0});
            MC_HIP(hipGetLastError());
            ctx->sh_pending = MC_SHARD_FOREST;
            if (ctx->comm) shard_drain_native(ctx);  // the forests over RCCL, then the rest of S6
            return;
        }
        s6_levels(ctx, false);
    });
}

int mc_cluster_set_edge_capture(mc_ctx *ctx, int64_t capacity)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(capacity >= 0, MC_ERR_INVALID, "negative capacity");
        ctx->cap_edges = capacity;
    });
}

int mc_cluster_get_edges(mc_ctx *ctx, uint64_t *keys, int64_t *n)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_cluster && n, MC_ERR_STATE, "no clustering result");
        MC_REQUIRE(ctx->cap_edges > 0, MC_ERR_STATE, "edge capture is off");
        unsigned long long cnt = 0;
        fetch(ctx, &cnt, ctx->d_cap_cnt.ptr, 8);
        *n = static_cast<int64_t>(cnt);
        if (keys && cnt) {
            MC_REQUIRE(static_cast<int64_t>(cnt) <= ctx->cap_edges, MC_ERR_UNSUPPORTED,
                       "more edges than the capture capacity (raise it and run again)");
            fetch(ctx, keys, ctx->d_cap_buf.ptr, cnt * 8);
        }
    });
}

int mc_cluster_get_info(mc_ctx *ctx, mc_cluster_info *info)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_cluster && info, MC_ERR_STATE, "no clustering result");
        sync_stats(ctx);
        info->num_iterations = ctx->n_iter;
        info->num_objects = ctx->h_stats[ST_K];
        info->num_nodes0 = ctx->N0;
        info->reserved = 0;
        info->num_object_points = ctx->h_stats[ST_NPTS];
        std::vector<int> len(std::max(ctx->K, 1));
        fetch(ctx, len.data(), ctx->fin.len, ctx->K * 4);
        int64_t tot = 0;
        for (int k = 0; k < ctx->K; k++) tot += len[k];
        info->num_object_contained = tot;
        info->num_object_masks = ctx->N0;
    });
}

int mc_cluster_get_level_sizes(mc_ctx *ctx, int32_t *sizes)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_cluster, MC_ERR_STATE, "no clustering result");
        fetch(ctx, sizes, ctx->d_Nlev.ptr, (ctx->n_iter + 1) * 4);
    });
}

int mc_cluster_get_level_caps(mc_ctx *ctx, int32_t *caps)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_cluster, MC_ERR_STATE, "no clustering result");
        fetch(ctx, caps, ctx->d_cap.ptr, (ctx->n_iter + 1) * 4);
    });
}

int mc_cluster_get_partition(mc_ctx *ctx, int32_t iteration, int32_t *labels)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_cluster, MC_ERR_STATE, "no clustering result");
        MC_REQUIRE(iteration >= 0 && iteration < ctx->n_iter, MC_ERR_INVALID, "iteration out of range");
        int nt = 0;
        fetch(ctx, &nt, ctx->d_Nlev.as<int>() + iteration, 4);
        const size_t n0 = static_cast<size_t>(std::max(ctx->N0, 1));
        fetch(ctx, labels, ctx->d_levels.as<int>() + static_cast<size_t>(iteration) * n0, nt * 4);
    });
}

int mc_cluster_get_edge_counts(mc_ctx *ctx, int64_t *edges)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_cluster, MC_ERR_STATE, "no clustering result");
        const size_t per = static_cast<size_t>(mc::kSpread) * mc::kSpreadStrideL;
        std::vector<unsigned long long> h(static_cast<size_t>(ctx->n_iter) * per);
        fetch(ctx, h.data(), ctx->d_edges.ptr, h.size() * 8);
        for (int t = 0; t < ctx->n_iter; t++) {  // fold the spread slots
            unsigned long long v = 0;
            for (int k = 0; k < mc::kSpread; k++) v += h[t * per + k * mc::kSpreadStrideL];
            edges[t] = static_cast<int64_t>(v);
        }
    });
}

int mc_cluster_get_final_labels(mc_ctx *ctx, int32_t *labels)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_cluster, MC_ERR_STATE, "no clustering result");
        fetch(ctx, labels, ctx->d_final_label.ptr, ctx->N0 * 4);
    });
}

int mc_cluster_get_objects(mc_ctx *ctx, uint64_t *vf_bits, int64_t *c_off, int32_t *c_idx, int64_t *pt_off,
                           int32_t *pt_idx, int64_t *mask_off, int32_t *mask_idx)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_cluster, MC_ERR_STATE, "no clustering result");
        sync_stats(ctx);
        const int K = ctx->K, FW = ctx->FW;
        hipStream_t s = ctx->stream;
        std::vector<int> off(std::max(K, 1)), len(std::max(K, 1)), poff(K + 1);
        if (K) {
            MC_HIP(hipMemcpyAsync(off.data(), ctx->fin.off, K * 4, hipMemcpyDeviceToHost, s));
            MC_HIP(hipMemcpyAsync(len.data(), ctx->fin.len, K * 4, hipMemcpyDeviceToHost, s));
            MC_HIP(hipMemcpyAsync(poff.data(), ctx->d_ptoff_out.ptr, (K + 1) * 4, hipMemcpyDeviceToHost, s));
            if (vf_bits && FW) MC_HIP(hipMemcpyAsync(vf_bits, ctx->fin.vf, static_cast<size_t>(K) * FW * 8, hipMemcpyDeviceToHost, s));
        }
        MC_HIP(hipStreamSynchronize(s));
        if (c_off) {
            c_off[0] = 0;
            int64_t end = 0;
            for (int k = 0; k < K; k++) {
                c_off[k + 1] = c_off[k] + len[k];
                if (len[k]) end = std::max<int64_t>(end, static_cast<int64_t>(off[k]) + len[k]);
            }
            if (c_idx && end) {  // one copy of the pool span, rows gathered on the host
                std::vector<int> pool(end);
                fetch(ctx, pool.data(), ctx->fin.pool, end * 4);
                for (int k = 0; k < K; k++)
                    if (len[k]) memcpy(c_idx + c_off[k], pool.data() + off[k], static_cast<size_t>(len[k]) * 4);
            }
        }
        if (pt_off) {
            for (int k = 0; k <= K; k++) pt_off[k] = K ? poff[k] : 0;
            const int np = K ? poff[K] : 0;
            if (pt_idx && np) MC_HIP(hipMemcpyAsync(pt_idx, ctx->d_pts_out.ptr, static_cast<size_t>(np) * 4, hipMemcpyDeviceToHost, s));
        }
        MC_HIP(hipStreamSynchronize(s));
        if (mask_off) {
            // members of each object as ascending level-0 node ids (stable counting sort)
            std::vector<int> fl(std::max(ctx->N0, 1));
            if (ctx->N0) MC_HIP(hipMemcpy(fl.data(), ctx->d_final_label.ptr, ctx->N0 * 4, hipMemcpyDeviceToHost));
            std::vector<int64_t> cnt(K + 1, 0);
            for (int i = 0; i < ctx->N0; i++) cnt[fl[i] + 1]++;
            for (int k = 0; k < K; k++) cnt[k + 1] += cnt[k];
            for (int k = 0; k <= K; k++) mask_off[k] = cnt[k];
            if (mask_idx)
                for (int i = 0; i < ctx->N0; i++) mask_idx[cnt[fl[i]]++] = i;
        }
    });
}

}  // extern "C"
