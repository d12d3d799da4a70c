// mc_shard_host.inl — row-block sharding over processes: the host side (included by
// mc_api.hip, same translation unit; kernels in mc_shard_kernels.inl).  A sharded mc_graph_build /
// mc_cluster_run stops at an exchange (shard.pending); shard_export packs this rank's block and
// shard_import takes all ranks' blocks and runs the next steps of mc_graph_host.inl /
// mc_cluster_host.inl.  The host moves the blocks (mc_shard_export / mc_shard_import), or, with a
// communicator attached, shard_drain_native does over RCCL, loaded on first use.
namespace {

bool sharded(const mc_ctx *ctx) { return ctx->shard.world > 1 || ctx->shard.comm; }

// this context is `rank` of `world` from now on: no exchange pending, its rows and S3 lists rebuilt
void shard_reset(mc_ctx *ctx, int rank, int world)
{
    SceneState &sc = ctx->scene;
    ShardState &sh = ctx->shard;
    sh.rank = rank;
    sh.world = world;
    sh.pending = 0;
    if (sc.have) build_s3_lists(ctx, mc::frame_starts(sc.h_col.data(), sc.M, sc.F));
}

void shard_export(mc_ctx *ctx, int32_t phase, void *dst_dev, int64_t *bytes)
{
    GraphState &gr = ctx->graph;
    ClusterState &cl = ctx->cluster;
    ShardState &sh = ctx->shard;
    MC_REQUIRE(bytes, MC_ERR_INVALID, "null bytes");
    MC_REQUIRE(phase == sh.pending && phase != 0, MC_ERR_STATE, "no such exchange pending");
    hipStream_t s = ctx->stream;
    if (phase == MC_SHARD_S3) {
        const int nr = sh.r1 - sh.r0;
        if (sh.s3_words < 0) {  // entry offsets of this rank's rows + their total (one host sync)
            sh.d_eoff.reserve((nr + 2) * 4);
            DevBuf dt;
            dt.reserve(8);
            mc::scan_device_n(s, gr.d_crow_len.as<int>() + sh.r0, sh.d_eoff.as<int>(), nullptr, nr,
                              dt.as<int>());
            int h = 0;
            MC_HIP(hipMemcpyAsync(&h, dt.ptr, 4, hipMemcpyDeviceToHost, s));
            MC_HIP(hipStreamSynchronize(s));
            sh.s3_words = 2 + 2 * static_cast<int64_t>(nr) + h;
        }
        *bytes = 4 * sh.s3_words;
        if (dst_dev)
            hipLaunchKernelGGL(mc::k_sh_s3_pack, grid_for(std::max(nr, 1) * 64, 256, 2048), dim3(256), 0, s,
                               sh.r0, sh.r1, ctx->scene.F, gr.d_ctmp.as<int>(), gr.d_crow_len.as<int>(),
                               gr.d_useg.as<unsigned char>(), sh.d_eoff.as<int>(), static_cast<int *>(dst_dev));
    } else if (phase == MC_SHARD_HIST) {
        *bytes = 8 * static_cast<int64_t>(ctx->scene.F + 1);
        if (dst_dev)
            MC_HIP(hipMemcpyAsync(dst_dev, gr.d_hist.ptr, *bytes, hipMemcpyDeviceToDevice, s));
    } else if (phase == MC_SHARD_FOREST) {
        *bytes = 4 * (static_cast<int64_t>(gr.N0) + 2);
        if (dst_dev)
            hipLaunchKernelGGL(mc::k_sh_forest_export, grid_for(gr.N0), dim3(256), 0, s, cl.d_Nlev.as<int>(),
                               cl.d_parent.as<int>(), cl.d_edges.as<unsigned long long>(),
                               static_cast<int *>(dst_dev), gr.N0);
    } else {
        throw McError{MC_ERR_INVALID, "unknown exchange phase"};
    }
    MC_HIP(hipGetLastError());
}

void shard_import(mc_ctx *ctx, int32_t phase, const void *src_dev, int64_t stride_bytes)
{
    GraphState &gr = ctx->graph;
    ClusterState &cl = ctx->cluster;
    ShardState &sh = ctx->shard;
    MC_REQUIRE(phase == sh.pending && phase != 0, MC_ERR_STATE, "no such exchange pending");
    MC_REQUIRE(src_dev, MC_ERR_INVALID, "null source");
    hipStream_t s = ctx->stream;
    const int W = sh.world;
    if (phase == MC_SHARD_S3) {
        MC_REQUIRE(stride_bytes % 4 == 0 && stride_bytes >= 8, MC_ERR_INVALID, "bad S3 block stride");
        hipLaunchKernelGGL(mc::k_sh_s3_unpack, dim3(mc::kUnpackWg, W), dim3(256), 0, s,
                           static_cast<const int *>(src_dev), static_cast<long long>(stride_bytes / 4), sh.rank,
                           ctx->scene.F, gr.d_ctmp.as<int>(), gr.d_crow_len.as<int>(), gr.d_useg.as<unsigned char>());
        MC_HIP(hipGetLastError());
        sh.pending = MC_SHARD_HIST;
        graph_undo_s5_hist(ctx);  // undo + S5 replicated, this rank's S4 tiles
    } else if (phase == MC_SHARD_HIST) {
        // src: the histogram summed over the ranks
        MC_HIP(hipMemcpyAsync(gr.d_hist.ptr, src_dev, 8 * static_cast<size_t>(ctx->scene.F + 1), hipMemcpyDeviceToDevice,
                              s));
        sh.pending = 0;
        graph_thresholds(ctx);
    } else if (phase == MC_SHARD_FOREST) {
        MC_REQUIRE(stride_bytes % 4 == 0 && stride_bytes >= 4 * (static_cast<int64_t>(gr.N0) + 2), MC_ERR_INVALID,
                   "bad FOREST block stride");
        {
            TimedScope ts(ctx->timer, s, "s6_pairs");
            hipLaunchKernelGGL(mc::k_sh_forest_import, dim3(grid_for(gr.N0, 256, 1024).x, W), dim3(256), 0, s,
                               cl.d_Nlev.as<int>(), static_cast<const int *>(src_dev),
                               static_cast<long long>(stride_bytes / 4), sh.rank, gr.N0,
                               cl.d_parent.as<int>(), cl.d_edges.as<unsigned long long>());
        }
        MC_HIP(hipGetLastError());
        sh.pending = 0;
        s6_levels(ctx, true);  // level 0's pairs are done: every rank's share, united above
    } else {
        throw McError{MC_ERR_INVALID, "unknown exchange phase"};
    }
}

// ---- native collectives: RCCL, loaded on first use ------------------------------------------
struct Rccl {
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) comm_init_rank = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclCommCount) comm_count = nullptr;
    decltype(&ncclCommUserRank) comm_user_rank = nullptr;
    decltype(&ncclAllReduce) all_reduce = nullptr;
    decltype(&ncclAllGather) all_gather = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
};

const Rccl *rccl_lib()
{
    static const Rccl r = [] {
        Rccl x;
        void *h = nullptr;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) return x;
        x.get_unique_id = reinterpret_cast<decltype(x.get_unique_id)>(dlsym(h, "ncclGetUniqueId"));
        x.comm_init_rank = reinterpret_cast<decltype(x.comm_init_rank)>(dlsym(h, "ncclCommInitRank"));
        x.comm_destroy = reinterpret_cast<decltype(x.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
        x.comm_count = reinterpret_cast<decltype(x.comm_count)>(dlsym(h, "ncclCommCount"));
        x.comm_user_rank = reinterpret_cast<decltype(x.comm_user_rank)>(dlsym(h, "ncclCommUserRank"));
        x.all_reduce = reinterpret_cast<decltype(x.all_reduce)>(dlsym(h, "ncclAllReduce"));
        x.all_gather = reinterpret_cast<decltype(x.all_gather)>(dlsym(h, "ncclAllGather"));
        x.error_string = reinterpret_cast<decltype(x.error_string)>(dlsym(h, "ncclGetErrorString"));
        return x;
    }();
    MC_REQUIRE(r.get_unique_id && r.comm_init_rank && r.comm_destroy && r.comm_count && r.comm_user_rank &&
                   r.all_reduce && r.all_gather && r.error_string,
               MC_ERR_UNSUPPORTED, "RCCL (librccl.so.1) not loadable");
    return &r;
}

void rccl_check(ncclResult_t e, const char *what)
{
    if (e != ncclSuccess) throw McError{MC_ERR_HIP, std::string(what) + ": " + rccl_lib()->error_string(e)};
}

// every pending exchange over the attached communicator, stream-ordered on the context stream:
// the S3 and FOREST blocks all-gathered into [world][stride] (S3's stride from a max all-reduce of
// the block sizes, one host read), the HIST block all-reduced (sum, int64)
void shard_drain_native(mc_ctx *ctx)
{
    ShardState &sh = ctx->shard;
    const Rccl &r = *rccl_lib();
    hipStream_t s = ctx->stream;
    auto comm = static_cast<ncclComm_t>(sh.comm);
    const size_t W = static_cast<size_t>(sh.world);
    while (sh.pending) {
        const int ph = sh.pending;
        int64_t bytes = 0;
        shard_export(ctx, ph, nullptr, &bytes);
        if (ph == MC_SHARD_HIST) {
            const size_t n = static_cast<size_t>(bytes) / 8;
            sh.d_send.reserve(n * 8);
            sh.d_recv.reserve(n * 8);
            shard_export(ctx, ph, sh.d_send.ptr, &bytes);
            rccl_check(r.all_reduce(sh.d_send.ptr, sh.d_recv.ptr, n, ncclInt64, ncclSum, comm, s),
                       "ncclAllReduce (observer histogram)");
            shard_import(ctx, ph, sh.d_recv.ptr, 0);
            continue;
        }
        int64_t n_max = bytes;
        if (ph == MC_SHARD_S3) {
            sh.d_size.reserve(8);
            MC_HIP(hipMemcpy(sh.d_size.ptr, &bytes, 8, hipMemcpyHostToDevice));  // done at return
            rccl_check(r.all_reduce(sh.d_size.ptr, sh.d_size.ptr, 1, ncclInt64, ncclMax, comm, s),
                       "ncclAllReduce (S3 block size)");
            MC_HIP(hipMemcpyAsync(&n_max, sh.d_size.ptr, 8, hipMemcpyDeviceToHost, s));
            MC_HIP(hipStreamSynchronize(s));
        }
        const size_t words = static_cast<size_t>(std::max<int64_t>((n_max + 3) / 4, 1));
        sh.d_send.reserve(words * 4);
        sh.d_recv.reserve(W * words * 4);
        MC_HIP(hipMemsetAsync(sh.d_send.ptr, 0, words * 4, s));
        shard_export(ctx, ph, sh.d_send.ptr, &bytes);
        rccl_check(r.all_gather(sh.d_send.ptr, sh.d_recv.ptr, words, ncclInt32, comm, s),
                   ph == MC_SHARD_S3 ? "ncclAllGather (S3 rows)" : "ncclAllGather (union-find forests)");
        shard_import(ctx, ph, sh.d_recv.ptr, static_cast<int64_t>(4 * words));
    }
}

void comm_detach(mc_ctx *ctx)
{
    ShardState &sh = ctx->shard;
    if (sh.comm && sh.own_comm) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)rccl_lib()->comm_destroy(static_cast<ncclComm_t>(sh.comm));
    }
    sh.comm = nullptr;
    sh.own_comm = false;
}

void comm_attach(mc_ctx *ctx, void *comm, bool own)
{
    int rank = 0, world = 1;
    rccl_check(rccl_lib()->comm_user_rank(static_cast<ncclComm_t>(comm), &rank), "ncclCommUserRank");
    rccl_check(rccl_lib()->comm_count(static_cast<ncclComm_t>(comm), &world), "ncclCommCount");
    comm_detach(ctx);
    ctx->shard.comm = comm;
    ctx->shard.own_comm = own;
    shard_reset(ctx, rank, world);
}

}  // namespace

extern "C" {

int mc_shard_set(mc_ctx *ctx, int32_t rank, int32_t world)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(world >= 1 && world <= 1024 && rank >= 0 && rank < world, MC_ERR_INVALID, "bad rank / world");
        MC_REQUIRE(!ctx->shard.comm, MC_ERR_STATE,
                   "a communicator is attached (rank / world come from it; detach first)");
        shard_reset(ctx, rank, world);
    });
}

int mc_shard_pending(mc_ctx *ctx, int32_t *phase)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(phase, MC_ERR_INVALID, "null phase");
        *phase = ctx->shard.pending;
    });
}

int mc_shard_export(mc_ctx *ctx, int32_t phase, void *dst_dev, int64_t *bytes)
{
    return guarded(ctx, [&] { shard_export(ctx, phase, dst_dev, bytes); });
}

int mc_shard_import(mc_ctx *ctx, int32_t phase, const void *src_dev, int64_t stride_bytes)
{
    return guarded(ctx, [&] { shard_import(ctx, phase, src_dev, stride_bytes); });
}

int mc_comm_unique_id(uint8_t id[MC_COMM_ID_BYTES])
{
    static_assert(MC_COMM_ID_BYTES == sizeof(ncclUniqueId), "unique id size");
    if (!id) return MC_ERR_INVALID;
    try {
        ncclUniqueId u;
        rccl_check(rccl_lib()->get_unique_id(&u), "ncclGetUniqueId");
        memcpy(id, &u, sizeof(u));
        return MC_OK;
    } catch (const McError &e) {
        return e.code;
    }
}

int mc_ctx_comm_init(mc_ctx *ctx, const uint8_t id[MC_COMM_ID_BYTES], int32_t rank, int32_t world)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(id, MC_ERR_INVALID, "null unique id");
        MC_REQUIRE(world >= 1 && world <= 1024 && rank >= 0 && rank < world, MC_ERR_INVALID, "bad rank / world");
        MC_HIP(hipSetDevice(ctx->device));
        ncclUniqueId u;
        memcpy(&u, id, sizeof(u));
        ncclComm_t c = nullptr;
        rccl_check(rccl_lib()->comm_init_rank(&c, world, u, rank), "ncclCommInitRank");
        comm_attach(ctx, c, true);
    });
}

int mc_ctx_attach_comm(mc_ctx *ctx, void *nccl_comm)
{
    return guarded(ctx, [&] {
        if (!nccl_comm) {
            comm_detach(ctx);
            shard_reset(ctx, 0, 1);
            return;
        }
        comm_attach(ctx, nccl_comm, false);
    });
}

}  // extern "C"
