// mc_cluster_host.inl — S6 iterative clustering and S7 final point sets: the host side (included by
// mc_api.hip, same translation unit).  One mc_cluster_run is s6_reserve, s6_init, s6_level0_columns,
// then s6_levels: per level s6_pairs (or s6_pairs_dense), s6_components and s6_merge, and after the
// last level s7_ranges and s7_points.  A sharded context runs level 0's pairs on its own rows, hands
// the forest to the exchange (mc_shard_host.inl) and enters s6_levels with the pairs done.  The mode
// and the components route are mc_graph_plan.hpp's.
namespace {

// level 0: the nodes' buffers
S6Level s6_level0(const GraphState &gr)
{
    return {gr.d_n0_off.as<int>(), gr.d_n0_len.as<int>(), gr.n0_pool, gr.d_owner0.as<int>(),
            gr.d_n0_vf.as<unsigned long long>()};
}

// the arrays level t's merge writes level t + 1 to: the A and B pools in turn
S6Level s6_level_after(const ClusterState &cl, int t)
{
    if (t % 2 == 0)
        return {cl.d_offA.as<int>(), cl.d_lenA.as<int>(), cl.d_poolA.as<int>(), cl.d_ownA.as<int>(),
                cl.d_vfA.as<unsigned long long>()};
    return {cl.d_offB.as<int>(), cl.d_lenB.as<int>(), cl.d_poolB.as<int>(), cl.d_ownB.as<int>(),
            cl.d_vfB.as<unsigned long long>()};
}

mc::EdgeCap edge_cap(const ClusterState &cl)
{
    if (cl.cap_edges <= 0) return mc::EdgeCap{nullptr, nullptr, 0};
    return mc::EdgeCap{cl.d_cap_buf.as<unsigned long long>(), cl.d_cap_cnt.as<unsigned long long>(),
                       static_cast<long long>(cl.cap_edges)};
}

// the S6/S7 buffers for N0 nodes, nnzC0 contained entries and nthr levels
void s6_reserve(mc_ctx *ctx)
{
    GraphState &gr = ctx->graph;
    ClusterState &cl = ctx->cluster;
    hipStream_t s = ctx->stream;
    const int N0 = gr.N0, FW = ctx->scene.FW, Mn = gr.Mn, nthr = cl.nthr;
    const size_t n0 = static_cast<size_t>(std::max(N0, 1));
    const size_t cap = static_cast<size_t>(std::max<int64_t>(gr.nnzC0, 1));
    cl.d_parent.reserve(n0 * 4);
    cl.d_root.reserve(n0 * 4);
    cl.d_isroot.reserve(n0 * 4);
    cl.d_rank.reserve((n0 + 1) * 4);
    cl.d_label.reserve(n0 * 4);
    cl.d_levels.reserve(std::max<size_t>(1, static_cast<size_t>(nthr)) * n0 * 4);
    const bool fresh_memcnt = cl.d_memcnt.bytes < n0 * 4;
    cl.d_memcnt.reserve(n0 * 4);
    if (fresh_memcnt) MC_HIP(hipMemsetAsync(cl.d_memcnt.ptr, 0, cl.d_memcnt.bytes, s));  // kept zero by K9
    cl.d_memoff.reserve((n0 + 1) * 4);
    cl.d_ublen.reserve(n0 * 4);
    cl.d_newoff.reserve((n0 + 1) * 4);
    cl.d_members.reserve(n0 * 4);
    const bool fresh_colcnt = cl.d_colcnt.bytes < static_cast<size_t>(Mn + 1) * 4;
    cl.d_colcnt.reserve((Mn + 1) * 4);
    if (fresh_colcnt) MC_HIP(hipMemsetAsync(cl.d_colcnt.ptr, 0, cl.d_colcnt.bytes, s));  // kept zero by K3
    cl.d_coloff.reserve((Mn + 2) * 4);
    cl.d_collen.reserve((Mn + 1) * 4);
    cl.d_colnodes.reserve(cap * 4);
    if (!cl.d_ovf_n.ptr) {
        cl.d_ovf_n.reserve((1 + mc::kOvfSlots) * 4);  // [0] unused counter (K5 clears it), [1..] slot locks
        MC_HIP(hipMemsetAsync(cl.d_ovf_n.ptr, 0, (1 + mc::kOvfSlots) * 4, s));  // locks kept zero
    }
    constexpr int kOvfBlocks = mc::kOvfSlots;
    if (cl.scratch_n0 < N0) {
        cl.d_scratch.reserve(static_cast<size_t>(kOvfBlocks) * n0 * 4);
        cl.d_touched.reserve(static_cast<size_t>(kOvfBlocks) * n0 * 4);
        MC_HIP(hipMemsetAsync(cl.d_scratch.ptr, 0, static_cast<size_t>(kOvfBlocks) * n0 * 4, s));
        cl.scratch_n0 = N0;
    }
    cl.d_edges.reserve(static_cast<size_t>(std::max(nthr, 1)) * mc::kSpread * mc::kSpreadStrideL * 8);  // spread slots
    cl.d_Nlev.reserve((nthr + 2) * 4);
    cl.d_cap.reserve((nthr + 2) * 4);
    cl.d_final_label.reserve(n0 * 4);
    cl.d_poolA.reserve(cap * 4);
    cl.d_poolB.reserve(cap * 4);
    cl.d_ownA.reserve(cap * 4);
    cl.d_ownB.reserve(cap * 4);
    cl.d_offA.reserve(n0 * 4);
    cl.d_offB.reserve(n0 * 4);
    cl.d_lenA.reserve(n0 * 4);
    cl.d_lenB.reserve(n0 * 4);
    cl.d_vfA.reserve(n0 * FW * 8 + 8);
    cl.d_vfB.reserve(n0 * FW * 8 + 8);
    cl.d_pmin.reserve(n0 * 4);
    cl.d_pmax.reserve(n0 * 4);
    cl.d_nwords.reserve(n0 * 4);
    cl.d_woff.reserve((n0 + 1) * 4);
    cl.d_ptcnt.reserve(n0 * 4);
    cl.d_ptoff_out.reserve((n0 + 1) * 4);
    cl.d_pts_out.reserve((gr.n0_pts_total + 1) * 4);
}

// level sizes, pool capacities, labels and edge counters at their start; the edge capture emptied
void s6_init(mc_ctx *ctx)
{
    GraphState &gr = ctx->graph;
    ClusterState &cl = ctx->cluster;
    hipStream_t s = ctx->stream;
    const int N0 = gr.N0, nthr = cl.nthr;
    int *stats = ctx->d_stats.as<int>();
    hipLaunchKernelGGL(mc::k6_init, grid_for(std::max<int64_t>(N0, nthr)), dim3(256), 0, s, N0,
                       cl.d_final_label.as<int>(), gr.nodes_from_graph ? stats + ST_N0 : nullptr, N0,
                       cl.d_Nlev.as<int>(), cl.d_cap.as<int>(), gr.nodes_from_graph ? stats + ST_NNZC : nullptr,
                       static_cast<int>(gr.nnzC0), cl.d_edges.as<unsigned long long>(), nthr);
    if (cl.cap_edges > 0) {
        cl.d_cap_buf.reserve(static_cast<size_t>(cl.cap_edges) * 8);
        cl.d_cap_cnt.reserve(8);
        MC_HIP(hipMemsetAsync(cl.d_cap_cnt.ptr, 0, 8, s));
    }
}

// level-0 column lists (nodes contained by each mask), for the sparse pairs
void s6_level0_columns(mc_ctx *ctx)
{
    GraphState &gr = ctx->graph;
    ClusterState &cl = ctx->cluster;
    if (cl.dense_obs || cl.nthr <= 0) return;
    hipStream_t s = ctx->stream;
    const int N0 = gr.N0, Mn = gr.Mn;
    int *Nlev = cl.d_Nlev.as<int>(), *dcap = cl.d_cap.as<int>();
    const S6Level l0 = s6_level0(gr);
    const dim3 gE = grid_for(std::max<int64_t>(N0, gr.nnzC0)), gC = grid_for(std::max(N0, Mn), 64, 8192);
    TimedScope ts(ctx->timer, s, "s6_columns");
    hipLaunchKernelGGL(mc::k6_colcount, gE, dim3(256), 0, s, Nlev, dcap, l0.pool, l0.own, cl.d_parent.as<int>(),
                       cl.d_colcnt.as<int>());
    mc::scan_device_n(s, cl.d_colcnt.as<int>(), cl.d_coloff.as<int>(), nullptr, Mn, nullptr);
    hipLaunchKernelGGL(mc::k6_colscatter, gE, dim3(256), 0, s, dcap, l0.pool, l0.own, cl.d_coloff.as<int>(),
                       cl.d_colcnt.as<int>(), cl.d_colnodes.as<int>());
    hipLaunchKernelGGL(mc::k6_colupdate, gC, dim3(64), 0, s, Mn, Nlev, cl.d_coloff.as<int>(),
                       cl.d_collen.as<int>(), cl.d_colnodes.as<int>(), nullptr, cl.d_parent.as<int>());
}

// level t's sparse pairs over the pair rows of `rank` of `world` (0 of 1: all of them)
void s6_pairs(mc_ctx *ctx, int t, const S6Level &lv, int rank, int world, mc::EdgeCap cap)
{
    ClusterState &cl = ctx->cluster;
    hipStream_t s = ctx->stream;
    const int N0 = ctx->graph.N0;
    TimedScope ts(ctx->timer, s, "s6_pairs");
    const mc::OvfWork ow{cl.d_scratch.as<int>(), cl.d_touched.as<int>(), N0, cl.d_ovf_n.as<int>() + 1};
    hipLaunchKernelGGL(mc::k6_pairs, grid_for(N0, mc::kPairWaves, 2048), dim3(256), 0, s, cl.d_Nlev.as<int>() + t,
                       lv.off, lv.len, lv.pool, cl.d_coloff.as<int>(), cl.d_collen.as<int>(),
                       cl.d_colnodes.as<int>(), lv.vf, ctx->scene.FW, ctx->graph.d_thr.as<float>(), t, cl.ctf,
                       cl.d_parent.as<int>(), cl.d_edges.as<unsigned long long>(), ow, rank, world, cap);
}

// level t's pairs when every pair with enough observers is linked (connect_threshold <= 0)
void s6_pairs_dense(mc_ctx *ctx, int t, const S6Level &lv)
{
    ClusterState &cl = ctx->cluster;
    hipStream_t s = ctx->stream;
    const int *dN = cl.d_Nlev.as<int>() + t;
    TimedScope ts(ctx->timer, s, "s6_pairs");
    hipLaunchKernelGGL(mc::k6_parent_init, grid_for(ctx->graph.N0), dim3(256), 0, s, dN, cl.d_parent.as<int>());
    hipLaunchKernelGGL(mc::k6_pairs_dense, dim3(4096), dim3(256), 0, s, dN, lv.vf, ctx->scene.FW,
                       ctx->graph.d_thr.as<float>(), t, cl.d_parent.as<int>(), cl.d_edges.as<unsigned long long>(),
                       edge_cap(cl));
}

// connected components of level t's forest: labels, members and row offsets of level t + 1
void s6_components(mc_ctx *ctx, int t, const S6Level &lv)
{
    ClusterState &cl = ctx->cluster;
    hipStream_t s = ctx->stream;
    const int N0 = ctx->graph.N0;
    const int *dN = cl.d_Nlev.as<int>() + t;
    int *dNn = cl.d_Nlev.as<int>() + t + 1, *dcapn = cl.d_cap.as<int>() + t + 1;
    int *levels_t = cl.d_levels.as<int>() + static_cast<size_t>(t) * static_cast<size_t>(std::max(N0, 1));
    const dim3 gN = grid_for(N0);
    TimedScope ts(ctx->timer, s, "s6_components");
    if (mc::s6_components_fused(t, N0)) {  // N_t <= N_1, typically N0 / 8: one workgroup
        hipLaunchKernelGGL(mc::k6_components, dim3(1), dim3(1024), 0, s, dN, dNn, cl.d_parent.as<int>(),
                           cl.d_root.as<int>(), cl.d_rank.as<int>(), lv.len, cl.d_label.as<int>(), levels_t,
                           cl.d_memcnt.as<int>(), cl.d_memoff.as<int>(), cl.d_ublen.as<int>(),
                           cl.d_newoff.as<int>(), dcapn, cl.d_members.as<int>(), cl.d_ovf_n.as<int>());
        return;
    }
    hipLaunchKernelGGL(mc::k6_compress, gN, dim3(256), 0, s, dN, cl.d_parent.as<int>(), cl.d_root.as<int>(),
                       cl.d_isroot.as<int>(), cl.d_ublen.as<int>(), cl.d_ovf_n.as<int>());
    mc::scan_device_n(s, cl.d_isroot.as<int>(), cl.d_rank.as<int>(), dN, 0, dNn);
    hipLaunchKernelGGL(mc::k6_relabel, gN, dim3(256), 0, s, dN, cl.d_root.as<int>(), cl.d_rank.as<int>(), lv.len,
                       cl.d_label.as<int>(), levels_t, cl.d_memcnt.as<int>(), cl.d_ublen.as<int>());
    mc::scan_device_n(s, cl.d_memcnt.as<int>(), cl.d_memoff.as<int>(), dNn, 0, nullptr, cl.d_ublen.as<int>(),
                      cl.d_newoff.as<int>(), dcapn);
    hipLaunchKernelGGL(mc::k6_memscatter, gN, dim3(256), 0, s, dN, 0, cl.d_label.as<int>(), cl.d_memoff.as<int>(),
                       cl.d_memcnt.as<int>(), cl.d_members.as<int>(), nullptr);
}

// level t + 1's nodes from the components' members, + the next level's column lists (nodes
// containing each mask, relabelled)
void s6_merge(mc_ctx *ctx, int t, const S6Level &lv, const S6Level &nx)
{
    GraphState &gr = ctx->graph;
    ClusterState &cl = ctx->cluster;
    hipStream_t s = ctx->stream;
    const int *dNn = cl.d_Nlev.as<int>() + t + 1;
    const bool cols = !cl.dense_obs && t + 1 < cl.nthr;
    TimedScope ts(ctx->timer, s, "s6_merge");
    const mc::ColUpdate cu{gr.Mn, dNn, cl.d_coloff.as<int>(), cl.d_collen.as<int>(), cl.d_colnodes.as<int>(),
                           cols ? cl.d_label.as<int>() : nullptr, cl.d_parent.as<int>(), gr.N0,
                           cl.d_label.as<int>(), cl.d_final_label.as<int>()};
    hipLaunchKernelGGL(mc::k6_merge, grid_for(gr.N0, 1, 2048), dim3(256), 0, s, dNn, cl.d_memoff.as<int>(),
                       cl.d_members.as<int>(), lv.off, lv.len, lv.pool, lv.vf, ctx->scene.FW, cl.d_newoff.as<int>(),
                       nx.off, nx.len, nx.pool, nx.own, nx.vf, cu);
}

// S7 ranges (node.py:35): every object's point-id range and the words of its range bitmap, from the
// point lists (by_point; ST_OBJOVF tells of a point in more objects than that path holds) or from
// the nodes' point lists; the sizes come to the host
void s7_ranges(mc_ctx *ctx, bool by_point)
{
    SceneState &sc = ctx->scene;
    GraphState &gr = ctx->graph;
    ClusterState &cl = ctx->cluster;
    hipStream_t s = ctx->stream;
    const int N0 = gr.N0;
    const int *dK = cl.d_Nlev.as<int>() + cl.n_iter;
    int *stats = ctx->d_stats.as<int>();
    const dim3 gN = grid_for(N0);
    {
        TimedScope ts(ctx->timer, s, "s7_points");
        hipLaunchKernelGGL(mc::k7_reset, gN, dim3(256), 0, s, N0, cl.d_pmin.as<int>(), cl.d_pmax.as<int>());
        if (by_point) {
            hipLaunchKernelGGL(mc::k7_obj_of_mask, grid_for(sc.M), dim3(256), 0, s, sc.M,
                               gr.d_node_of_mask.as<int>(), cl.d_final_label.as<int>(),
                               cl.d_obj_of_mask.as<int>());
            hipLaunchKernelGGL(mc::k7p_points<0>, dim3(ceil_div(sc.P, 256)), dim3(256), 0, s, static_cast<int>(sc.P),
                               gr.d_pt_off.as<int>(), gr.d_pt_list.as<unsigned>(), sc.d_frame_start.as<int>(),
                               cl.d_obj_of_mask.as<int>(), cl.d_pmin.as<int>(), cl.d_pmax.as<int>(), nullptr,
                               nullptr, stats + ST_OBJOVF);
        } else {
            hipLaunchKernelGGL(mc::k7_minmax, grid_for(N0, mc::kPairWaves, 2048), dim3(256), 0, s, N0,
                               cl.d_final_label.as<int>(), gr.d_n0_ptoff.as<int>(), gr.d_n0_ptlen.as<int>(),
                               gr.n0_pts, cl.d_pmin.as<int>(), cl.d_pmax.as<int>());
        }
        hipLaunchKernelGGL(mc::k7_words, gN, dim3(256), 0, s, dK, cl.d_pmin.as<int>(), cl.d_pmax.as<int>(),
                           cl.d_nwords.as<int>(), stats + ST_K);
        mc::scan_device_n(s, cl.d_nwords.as<int>(), cl.d_woff.as<int>(), dK, 0, stats + ST_WORDS);
    }
    sync_stats(ctx);  // bitmap capacity
    cl.K = ctx->h_stats[ST_K];
}

// S7 points: the objects' range bitmaps set (by point or by node), counted and extracted
void s7_points(mc_ctx *ctx, bool by_point)
{
    SceneState &sc = ctx->scene;
    GraphState &gr = ctx->graph;
    ClusterState &cl = ctx->cluster;
    hipStream_t s = ctx->stream;
    const int N0 = gr.N0;
    const int *dK = cl.d_Nlev.as<int>() + cl.n_iter;
    int *stats = ctx->d_stats.as<int>();
    const dim3 gK = grid_for(N0, 1, 2048);
    const size_t words = static_cast<size_t>(std::max(ctx->h_stats[ST_WORDS], 1));
    cl.d_bm.reserve(words * 8);
    TimedScope ts(ctx->timer, s, "s7_points");
    MC_HIP(hipMemsetAsync(cl.d_bm.ptr, 0, words * 8, s));
    if (by_point)
        hipLaunchKernelGGL(mc::k7p_points<1>, dim3(ceil_div(sc.P, 256)), dim3(256), 0, s, static_cast<int>(sc.P),
                           gr.d_pt_off.as<int>(), gr.d_pt_list.as<unsigned>(), sc.d_frame_start.as<int>(),
                           cl.d_obj_of_mask.as<int>(), cl.d_pmin.as<int>(), cl.d_pmax.as<int>(),
                           cl.d_woff.as<int>(), cl.d_bm.as<unsigned long long>(), stats + ST_OBJOVF);
    else
        hipLaunchKernelGGL(mc::k7_setbits, grid_for(N0, mc::kPairWaves, 2048), dim3(256), 0, s, N0,
                           cl.d_final_label.as<int>(), gr.d_n0_ptoff.as<int>(), gr.d_n0_ptlen.as<int>(), gr.n0_pts,
                           cl.d_pmin.as<int>(), cl.d_woff.as<int>(), cl.d_bm.as<unsigned long long>());
    hipLaunchKernelGGL(mc::k7_count, gK, dim3(256), 0, s, dK, cl.d_woff.as<int>(), cl.d_bm.as<unsigned long long>(),
                       cl.d_ptcnt.as<int>());
    mc::scan_device_n(s, cl.d_ptcnt.as<int>(), cl.d_ptoff_out.as<int>(), dK, 0, stats + ST_NPTS);
    hipLaunchKernelGGL(mc::k7_extract, gK, dim3(256), 0, s, dK, cl.d_woff.as<int>(), cl.d_bm.as<unsigned long long>(),
                       cl.d_pmin.as<int>(), cl.d_ptoff_out.as<int>(), cl.d_pts_out.as<int>());
}

// the S6 levels (pairs0_done: level 0's pairs ran on every rank's rows and their forests were
// united) and the final objects with their point sets; level t + 1 lives in the ping-pong pools
void s6_levels(mc_ctx *ctx, bool pairs0_done)
{
    ClusterState &cl = ctx->cluster;
    S6Level lv = s6_level0(ctx->graph);
    for (int t = 0; t < cl.nthr; t++) {
        const S6Level nx = s6_level_after(cl, t);
        if (t > 0 || !pairs0_done) {
            if (cl.dense_obs) s6_pairs_dense(ctx, t, lv);
            else s6_pairs(ctx, t, lv, 0, 1, edge_cap(cl));
        }
        s6_components(ctx, t, lv);
        s6_merge(ctx, t, lv, nx);
        lv = nx;
    }
    cl.fin = lv;
    cl.n_iter = cl.nthr;
    const bool point_path = ctx->graph.nodes_from_graph;
    s7_ranges(ctx, point_path);
    const bool use_points = point_path && ctx->h_stats[ST_OBJOVF] == 0;
    if (point_path && !use_points) s7_ranges(ctx, false);  // a point in > 8 objects: redo the ranges per node
    s7_points(ctx, use_points);
    MC_HIP(hipGetLastError());
    MC_HIP(hipMemcpyAsync(ctx->h_stats, ctx->d_stats.ptr, ST_COUNT * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    cl.have = true;
}

}  // namespace

extern "C" {

int mc_cluster_run(mc_ctx *ctx, const float *thresholds, int32_t n, double connect_threshold)
{
    return guarded(ctx, [&] {
        GraphState &gr = ctx->graph;
        ClusterState &cl = ctx->cluster;
        ShardState &sh = ctx->shard;
        MC_REQUIRE(gr.have_nodes, MC_ERR_STATE, "mc_cluster_run before mc_graph_build / mc_nodes_set");
        // (edge capture on a sharded context: iteration 0 evaluates only this rank's pair rows, so its
        // capture holds those rows' edges and the driver gathers them, graph_shard.ShardedGraph.edges;
        // the later iterations run replicated and every rank captures all of their edges)
        hipStream_t s = ctx->stream;
        if (gr.nodes_from_graph) {
            sync_stats(ctx);  // the one host round trip between S4 and S6 (sizes for the S6 buffers)
            gr.N0 = ctx->h_stats[ST_N0];
            gr.nnzC0 = ctx->h_stats[ST_NNZC];
        }
        int nthr;
        if (thresholds) {
            MC_REQUIRE(n >= 0 && n <= 4096, MC_ERR_INVALID, "bad threshold count");
            nthr = n;
            gr.d_thr.reserve((n + 1) * sizeof(float));
            if (n) MC_HIP(hipMemcpyAsync(gr.d_thr.ptr, thresholds, n * sizeof(float), hipMemcpyHostToDevice, s));
        } else {
            MC_REQUIRE(gr.nodes_from_graph, MC_ERR_STATE, "device thresholds need mc_graph_build");
            if (ctx->h_stats[ST_THR_STATUS] != MC_OK)
                throw McError{ctx->h_stats[ST_THR_STATUS], "no positive observer count (np.percentile of an empty array)"};
            nthr = ctx->h_stats[ST_NTHR];
        }
        const int N0 = gr.N0;
        MC_REQUIRE(!(N0 == 0 && nthr > 0), MC_ERR_NO_NODES, "no nodes to cluster (torch.stack of an empty list)");
        const mc::S6Mode mode = mc::s6_mode(connect_threshold);
        cl.nthr = nthr;
        cl.dense_obs = mode.dense_obs;
        cl.ctf = mode.ctf;
        s6_reserve(ctx);
        s6_init(ctx);
        s6_level0_columns(ctx);
        cl.have = false;
        sh.pending = 0;
        if (nthr > 0 && N0 > 0 && sharded(ctx) && !mode.dense_obs) {
            // iteration 0 (the N0 x N0 pairs) on this rank's rows; the union-find forests of all
            // ranks are united by mc_shard_import(MC_SHARD_FOREST), which runs the rest
            s6_pairs(ctx, 0, s6_level0(gr), sh.rank, sh.world, mc::EdgeCap{nullptr, nullptr, 0});
            MC_HIP(hipGetLastError());
            sh.pending = MC_SHARD_FOREST;
            if (sh.comm) shard_drain_native(ctx);  // the forests over RCCL, then the rest of S6
            return;
        }
        s6_levels(ctx, false);
    });
}

int mc_cluster_set_edge_capture(mc_ctx *ctx, int64_t capacity)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(capacity >= 0, MC_ERR_INVALID, "negative capacity");
        ctx->cluster.cap_edges = capacity;
    });
}

int mc_cluster_get_edges(mc_ctx *ctx, uint64_t *keys, int64_t *n)
{
    return guarded(ctx, [&] {
        ClusterState &cl = ctx->cluster;
        MC_REQUIRE(cl.have && n, MC_ERR_STATE, "no clustering result");
        MC_REQUIRE(cl.cap_edges > 0, MC_ERR_STATE, "edge capture is off");
        unsigned long long cnt = 0;
        fetch(ctx, &cnt, cl.d_cap_cnt.ptr, 8);
        *n = static_cast<int64_t>(cnt);
        if (keys && cnt) {
            MC_REQUIRE(static_cast<int64_t>(cnt) <= cl.cap_edges, MC_ERR_UNSUPPORTED,
                       "more edges than the capture capacity (raise it and run again)");
            fetch(ctx, keys, cl.d_cap_buf.ptr, cnt * 8);
        }
    });
}

int mc_cluster_get_info(mc_ctx *ctx, mc_cluster_info *info)
{
    return guarded(ctx, [&] {
        ClusterState &cl = ctx->cluster;
        MC_REQUIRE(cl.have && info, MC_ERR_STATE, "no clustering result");
        sync_stats(ctx);
        info->num_iterations = cl.n_iter;
        info->num_objects = ctx->h_stats[ST_K];
        info->num_nodes0 = ctx->graph.N0;
        info->reserved = 0;
        info->num_object_points = ctx->h_stats[ST_NPTS];
        std::vector<int> len(std::max(cl.K, 1));
        fetch(ctx, len.data(), cl.fin.len, cl.K * 4);
        int64_t tot = 0;
        for (int k = 0; k < cl.K; k++) tot += len[k];
        info->num_object_contained = tot;
        info->num_object_masks = ctx->graph.N0;
    });
}

int mc_cluster_get_level_sizes(mc_ctx *ctx, int32_t *sizes)
{
    return guarded(ctx, [&] {
        ClusterState &cl = ctx->cluster;
        MC_REQUIRE(cl.have, MC_ERR_STATE, "no clustering result");
        fetch(ctx, sizes, cl.d_Nlev.ptr, (cl.n_iter + 1) * 4);
    });
}

int mc_cluster_get_level_caps(mc_ctx *ctx, int32_t *caps)
{
    return guarded(ctx, [&] {
        ClusterState &cl = ctx->cluster;
        MC_REQUIRE(cl.have, MC_ERR_STATE, "no clustering result");
        fetch(ctx, caps, cl.d_cap.ptr, (cl.n_iter + 1) * 4);
    });
}

int mc_cluster_get_partition(mc_ctx *ctx, int32_t iteration, int32_t *labels)
{
    return guarded(ctx, [&] {
        ClusterState &cl = ctx->cluster;
        MC_REQUIRE(cl.have, MC_ERR_STATE, "no clustering result");
        MC_REQUIRE(iteration >= 0 && iteration < cl.n_iter, MC_ERR_INVALID, "iteration out of range");
        int nt = 0;
        fetch(ctx, &nt, cl.d_Nlev.as<int>() + iteration, 4);
        const size_t n0 = static_cast<size_t>(std::max(ctx->graph.N0, 1));
        fetch(ctx, labels, cl.d_levels.as<int>() + static_cast<size_t>(iteration) * n0, nt * 4);
    });
}

int mc_cluster_get_edge_counts(mc_ctx *ctx, int64_t *edges)
{
    return guarded(ctx, [&] {
        ClusterState &cl = ctx->cluster;
        MC_REQUIRE(cl.have, MC_ERR_STATE, "no clustering result");
        const size_t per = static_cast<size_t>(mc::kSpread) * mc::kSpreadStrideL;
        std::vector<unsigned long long> h(static_cast<size_t>(cl.n_iter) * per);
        fetch(ctx, h.data(), cl.d_edges.ptr, h.size() * 8);
        for (int t = 0; t < cl.n_iter; t++) {  // fold the spread slots
            unsigned long long v = 0;
            for (int k = 0; k < mc::kSpread; k++) v += h[t * per + k * mc::kSpreadStrideL];
            edges[t] = static_cast<int64_t>(v);
        }
    });
}

int mc_cluster_get_final_labels(mc_ctx *ctx, int32_t *labels)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->cluster.have, MC_ERR_STATE, "no clustering result");
        fetch(ctx, labels, ctx->cluster.d_final_label.ptr, ctx->graph.N0 * 4);
    });
}

int mc_cluster_get_objects(mc_ctx *ctx, uint64_t *vf_bits, int64_t *c_off, int32_t *c_idx, int64_t *pt_off,
                           int32_t *pt_idx, int64_t *mask_off, int32_t *mask_idx)
{
    return guarded(ctx, [&] {
        GraphState &gr = ctx->graph;
        ClusterState &cl = ctx->cluster;
        MC_REQUIRE(cl.have, MC_ERR_STATE, "no clustering result");
        sync_stats(ctx);
        const int K = cl.K, FW = ctx->scene.FW;
        hipStream_t s = ctx->stream;
        std::vector<int> off(std::max(K, 1)), len(std::max(K, 1)), poff(K + 1);
        if (K) {
            MC_HIP(hipMemcpyAsync(off.data(), cl.fin.off, K * 4, hipMemcpyDeviceToHost, s));
            MC_HIP(hipMemcpyAsync(len.data(), cl.fin.len, K * 4, hipMemcpyDeviceToHost, s));
            MC_HIP(hipMemcpyAsync(poff.data(), cl.d_ptoff_out.ptr, (K + 1) * 4, hipMemcpyDeviceToHost, s));
            if (vf_bits && FW) MC_HIP(hipMemcpyAsync(vf_bits, cl.fin.vf, static_cast<size_t>(K) * FW * 8, hipMemcpyDeviceToHost, s));
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
                fetch(ctx, pool.data(), cl.fin.pool, end * 4);
                for (int k = 0; k < K; k++)
                    if (len[k]) memcpy(c_idx + c_off[k], pool.data() + off[k], static_cast<size_t>(len[k]) * 4);
            }
        }
        if (pt_off) {
            for (int k = 0; k <= K; k++) pt_off[k] = K ? poff[k] : 0;
            const int np = K ? poff[K] : 0;
            if (pt_idx && np) MC_HIP(hipMemcpyAsync(pt_idx, cl.d_pts_out.ptr, static_cast<size_t>(np) * 4, hipMemcpyDeviceToHost, s));
        }
        MC_HIP(hipStreamSynchronize(s));
        if (mask_off) {
            // members of each object as ascending level-0 node ids (stable counting sort)
            std::vector<int> fl(std::max(gr.N0, 1));
            if (gr.N0) MC_HIP(hipMemcpy(fl.data(), cl.d_final_label.ptr, gr.N0 * 4, hipMemcpyDeviceToHost));
            std::vector<int64_t> cnt(K + 1, 0);
            for (int i = 0; i < gr.N0; i++) cnt[fl[i] + 1]++;
            for (int k = 0; k < K; k++) cnt[k + 1] += cnt[k];
            for (int k = 0; k <= K; k++) mask_off[k] = cnt[k];
            if (mask_idx)
                for (int i = 0; i < gr.N0; i++) mask_idx[cnt[fl[i]]++] = i;
        }
    });
}

}  // extern "C"
