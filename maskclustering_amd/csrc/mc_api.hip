// mc_api.hip — C-ABI of libmcgraph: context, scene upload, S2–S6 orchestration, getters.
// Single translation unit: the kernels live in mc_kernels.inl.
#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the library loads RCCL at mc_ctx_attach_comm / mc_ctx_comm_init (dlopen)

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "mc_internal.hpp"
#include "mc_bp_plan.hpp"
#include "mc_pp_plan.hpp"
#include "mc_kernels.inl"
#include "mc_bp_kernels.inl"
#include "mc_pp_kernels.inl"
#include "mc_eval_kernels.inl"
#include "mc_ap_kernels.inl"
#include "mc_io_kernels.inl"
#include "mc_shard_kernels.inl"
#include "mc_ov_kernels.inl"
#include "mc_setorder.inl"

using mc::DevBuf;
using mc::McError;
using mc::TimedScope;
using mc::ceil_div;

namespace {

// device-side statistics block (copied to pinned host memory in one transfer)
enum Stat : int {
    ST_NBND = 0,      // boundary points
    ST_NNZC = 1,      // contained entries after undo
    ST_N0 = 2,        // level-0 nodes
    ST_NTHR = 3,      // thresholds
    ST_THR_STATUS = 4,
    ST_K = 5,         // final objects
    ST_WORDS = 6,     // point-bitmap words
    ST_NPTS = 7,      // object points (sum)
    ST_OBJOVF = 8,    // a point in more objects than the per-point fast path holds
    ST_COUNT = 9,
};

// S6 levels t >= 1 of scenes with at most this many level-0 nodes run the component labelling in
// one workgroup (k6_components, one launch); level 0 and larger scenes use the multi-workgroup
// kernels (k6_compress .. k6_memscatter, five launches)
constexpr int kFusedComponentsMaxN0 = 32768;

// MC_STAGE_THREADS: host threads of the staging copies (mc_backproject_frames, mc_bits_unpack)
int stage_threads_knob(int dflt)
{
    if (const char *e = getenv("MC_STAGE_THREADS")) return std::max(1, std::min(64, atoi(e)));
    return dflt;
}

// S1 back-projection state of a context (the host code is mc_bp_host.inl)
struct BpState {
    // scene points and their 2r grid
    int64_t P = 0;
    bool have_points = false, have_result = false;
    float grid_radius = -1.f;  // scene grid built for this ball radius
    unsigned gnb = 0;
    DevBuf scene, gcnt, gstart, gbkt, gcellk, gpts, gidx, gcell, gscan_tmp;
    // frames that arrive from the host
    DevBuf in_depth, in_seg, in_intr, in_pose, in_raw;
    char *h_stage[2] = {nullptr, nullptr};  // pinned staging ring of mc_backproject_frames (two chunks, ping-pong)
    size_t stage_bytes = 0;
    hipEvent_t ev_stage[2] = {};
    bool stage_used[2] = {false, false};
    hipStream_t copy = nullptr;  // host frames staged batch by batch while the previous batch computes
    hipEvent_t ev_up = nullptr;
    // per-batch arrays
    DevBuf band, present, fflags, cand, npix, csidx, poff, slot_of, stat;
    DevBuf vid;  // valid-id map (k_bp_count -> k_bp_compact), 1 byte per pixel
    DevBuf slot_frame, slot_id, slot_np, slot_pix, slot_nv, slot_m, slot_ns, slot_box, slot_nn, slot_toff, slot_cov;
    DevBuf pix_list, hkey, hvid, hfirst, vox_entry, acc, vpts, pcell, pbkt, bcnt, bstart, blist, ncnt, par, droot, rnk,
        lab, ccnt, ssidx, avg, qpts;
    DevBuf bm, tmp, kflag, ksize, midx, moff, out_col, out_label, out_off;
    DevBuf cls_list, nbl, lean, vox_order;  // denoise size-class slot lists; per-workgroup eps-neighbour lists, lean scratch
    DevBuf vx_pvid, vx_list, vx_fb;  // voxel_down_sample: per-pixel voxel ids and voxel lists of k_bp_voxel_lds; its overflow slots
    DevBuf scanm;      // block sums of the multi-workgroup scans
    DevBuf slot_grid;  // denoise: grid origin / extent of the slots with points queued for the k-NN ring search
    DevBuf pack;       // the batch's readback, packed (k_bp_pack)
    int *h_pack = nullptr;  // its pinned copy, h_pack_n ints
    size_t h_pack_n = 0;
    hipEvent_t ev_pack = nullptr;  // the last batch's h_pack copy (appended under the next batch)
    int *h_stat = nullptr;         // pinned copy of the status block
    hipStream_t cls_stream[mc::kBpStreamClasses] = {};  // denoise: the LDS size classes run side by side
    hipEvent_t ev_cls[mc::kBpStreamClasses] = {};
    // batch sizing
    int64_t mem_budget = 0;  // bytes the per-batch arrays may take (0: the default share, mc_bp_plan.hpp)
    size_t px_cap = 0;       // mask-pixel capacity of the per-batch arrays (pixel-list positions)
    size_t fpx_cap = 0;      // frame-pixel capacity (the valid-id map)
    double mfrac = 1.0;      // mask pixels per frame pixel a batch is sized for (the largest seen, + margin)
    bool mfrac_obs = false;  // mfrac comes from an earlier call's batches (not the initial guess)
    int last_fb = 0;         // frames per batch at the end of the last call
    int64_t redo = 0;        // batches redone after a mask-pixel overflow (all calls)
    // results of the last call
    int F = 0, err_frame = -1;
    int64_t nnz = 0;
    DevBuf pts;  // the masks' point lists
    std::vector<int32_t> col, label, stats;
    std::vector<int64_t> off;
};

// AP evaluation state of a context (the host code is mc_ap_host.inl)
struct EvTables {  // one scan's compact tables (include/mcgraph.h, mc_ev_get_scan)
    std::vector<int32_t> gcls, gid, pcls, ppred, pgt;
    std::vector<int64_t> gvert, pvert, pvoid, pint;
    std::vector<double> pscore;
};

struct EvState {
    bool active = false;
    int C = 0, O = 0, nlab = 0;
    int64_t min_region = 100;
    bool no_class = false;
    std::vector<int32_t> class_ids;
    std::vector<double> overlaps;
    DevBuf d_lab2cls, d_overlaps;
    // accumulated over the scans: examples in per-unit regions, one unit per (scan, class, overlap)
    int64_t ex_used = 0;
    int units = 0;
    DevBuf d_ex_key, d_ex_true, d_unit_cell, d_unit_off, d_unit_cnt, d_hardfn, d_flags;
    EvTables last;
    bool have_last = false;
    // the table of the last mc_ev_ap
    bool ap_valid = false;
    std::vector<double> ap;
    std::vector<int64_t> stats;
    std::vector<int32_t> ndist;
    DevBuf d_key, d_true, d_prec, d_rec, d_cell, d_ap, d_stats, d_ndist;
    // scratch of one mc_ev_add_scan / commit
    std::vector<int64_t> h_out;
    DevBuf d_info, d_in[5], d_cnt, d_inst, d_tmp_id, d_class, d_gcls, d_gid, d_gvert, d_pinst, d_pk, d_pair_gt, d_pair_int,
        d_out, d_words, d_tmp;
};

}  // namespace

struct mc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t side = nullptr;                 // S3: workgroup-per-mask kernel beside the wave kernel
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::string err;
    mc::KernelTimer timer;
    int *h_stats = nullptr;  // pinned
    int num_cu = 256;
    BpState bp;  // S1 back-projection

    // ---- scene ----
    bool have_scene = false, have_graph = false, have_nodes = false, have_cluster = false;
    bool nodes_from_graph = false;
    int64_t P = 0;
    int F = 0, FW = 0, M = 0, M_in = 0;
    int nnz = 0;
    std::vector<int32_t> h_col, h_label, h_in_index, h_off;
    DevBuf d_mask_off, d_mask_pts, d_mask_col, d_mask_label, d_frame_start, d_valid;
    // ---- S2 ----
    DevBuf d_deg, d_pt_off, d_pt_list, d_boundary, d_pfm, d_scan_tmp;
    // ---- S3/S5 ----
    DevBuf d_ctmp, d_crow_len, d_useg, d_keep_cnt, d_node_flag, d_node_pos, d_c_off, d_c_idx, d_vf;
    // ---- S4 ----
    DevBuf d_hist, d_thr, d_isint, d_stats, d_s4rng;
    // ---- level-0 nodes ----
    int N0 = 0;        // host copy (valid after sync_stats or mc_nodes_set)
    int Mn = 0;        // mask-id space of C rows
    int64_t n0_pts_total = 0;
    DevBuf d_node0_g, d_n0_off, d_n0_len, d_n0_ptoff, d_n0_ptlen, d_n0_vf, d_user_cidx, d_user_pts;
    DevBuf d_owner0, d_node_of_mask, d_obj_of_mask, d_s3_small, d_s3_big, d_collen;
    int n_s3_small = 0, n_s3_big = 0;
    const int *n0_pool = nullptr;
    const int *n0_pts = nullptr;
    int64_t nnzC0 = 0;
    // ---- S6 ----
    DevBuf d_parent, d_root, d_isroot, d_rank, d_label, d_levels, d_memcnt, d_memoff, d_ublen, d_newoff;
    DevBuf d_members, d_colcnt, d_coloff, d_colnodes, d_ovf_n, d_scratch, d_touched, d_edges;
    DevBuf d_spread;  // spread slots of the S2 boundary counter
    DevBuf d_Nlev, d_final_label;
    DevBuf d_poolA, d_poolB, d_offA, d_offB, d_lenA, d_lenB, d_vfA, d_vfB, d_ownA, d_ownB, d_cap;
    DevBuf d_pmin, d_pmax, d_nwords, d_woff, d_bm, d_ptcnt, d_ptoff_out, d_pts_out;
    int scratch_n0 = -1;
    int n_iter = 0;
    // final object state (device pointers into the pools)
    const int *fin_off = nullptr, *fin_len = nullptr, *fin_pool = nullptr;
    const unsigned long long *fin_vf = nullptr;
    int K = 0;
    int64_t npts = 0;

    // ---- row-block sharding over processes ----
    int sh_rank = 0, sh_world = 1;
    int sh_pending = 0;          // MC_SHARD_* phase waiting for the host's exchange, 0 = none
    int sh_r0 = 0, sh_r1 = 0;    // this rank's S3 mask rows
    int64_t sh_s3_words = -1;    // size of this rank's S3 block (valid while sh_pending == MC_SHARD_S3)
    mc_graph_params sh_params{};
    DevBuf d_sh_eoff;
    // native collectives (mc_ctx_attach_comm / mc_ctx_comm_init): with a communicator attached the
    // sharded mc_graph_build / mc_cluster_run run their exchanges themselves, on the context stream
    void *comm = nullptr;        // ncclComm_t
    bool own_comm = false;
    DevBuf d_sh_send, d_sh_recv, d_sh_size;
    // S6 state kept across the FOREST exchange
    int s6_nthr = 0;
    bool s6_dense_obs = false;
    float s6_ctf = 0.f;
    // edge capture for the set-order replay (mc_cluster_set_edge_capture)
    int64_t cap_edges = 0;
    DevBuf d_cap_buf, d_cap_cnt;

    // ---- post-processing ----
    DevBuf d_pp_posmap;  // one P-entry position map per workgroup, -1 at rest
    int64_t pp_posmap_P = 0;
    int pp_posmap_slots = 0;
    bool have_pp = false;
    mc_pp_info pp_info{};
    std::vector<int32_t> pp_entry_obj, pp_qobj, pp_obj_node;
    std::vector<double> pp_qcov, pp_box;
    std::vector<uint8_t> pp_state;
    // the node arrays and per-entry results of the last run, resident for the export
    DevBuf d_pp_npoff, d_pp_npts, d_pp_qoff, d_pp_qm, d_pp_eobj, d_pp_qobj, d_pp_qcov;
    int64_t pp_P = 0;
    bool pp_host = false;    // pp_entry_obj / pp_qobj / pp_qcov are fetched (mc_pp_get_results)
    bool pp_export = false;  // the export arrays below are built
    std::vector<int32_t> pp_fslot, pp_fin, pp_fin_node;  // object -> final slot; final objects, their nodes
    std::vector<int64_t> pp_opoff, pp_omoff;             // point / mask list offsets of the final objects
    DevBuf d_pp_fslot, d_pp_finobj, d_pp_finnode, d_pp_opoff, d_pp_omoff, d_pp_opts, d_pp_omask, d_pp_ocov, d_pp_repre;

    EvState ev;  // AP evaluation (mc_ev_*)
};

namespace {

int fail(mc_ctx *ctx, const McError &e)
{
    if (ctx) ctx->err = e.msg;
    return e.code;
}

template <typename Fn>
int guarded(mc_ctx *ctx, Fn &&fn)
{
    if (!ctx) return MC_ERR_INVALID;
    try {
        MC_HIP(hipSetDevice(ctx->device));
        fn();
        return MC_OK;
    } catch (const McError &e) {
        return fail(ctx, e);
    } catch (const std::exception &e) {
        return fail(ctx, McError{MC_ERR_INVALID, e.what()});
    }
}

inline dim3 grid_for(int64_t n, int per_block = 256, int cap = 4096)
{
    int64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return dim3(static_cast<unsigned>(g));
}

void sync_stats(mc_ctx *ctx)
{
    MC_HIP(hipMemcpyAsync(ctx->h_stats, ctx->d_stats.ptr, ST_COUNT * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MC_HIP(hipStreamSynchronize(ctx->stream));
    ctx->timer.collect();
}


// S4 histogram launch: persistent blocks, R lane-indexed LDS replicas (odd stride)
// rng: >= ceil(M / 64) int2 of scratch
void launch_hist(hipStream_t s, const unsigned long long *vf, int M, int F, unsigned long long *hist, int2 *rng,
                 int shard_rank = 0, int shard_world = 1)
{
    if (!M || !F) return;
    const int FW = (F + 63) / 64;
    const int nblk = ceil_div(M, mc::kHistTile);
    hipLaunchKernelGGL(mc::k_s4_ranges, grid_for(static_cast<int64_t>(nblk) * 64), dim3(256), 0, s, vf, M, FW, nblk, rng);
    const long long ntiles = static_cast<long long>(nblk) * (nblk + 1) / 2;
    const int HS = (F + 1) | 1;
    int R = 32;
    while (R > 1 && static_cast<size_t>(R) * HS * 4 > 40 * 1024) R >>= 1;
    const size_t lds = 2 * mc::kHistTile * mc::kHistKW * sizeof(unsigned long long) + static_cast<size_t>(R) * HS * 4;
    const long long grid = std::min<long long>(ntiles, 1024);
    hipLaunchKernelGGL(mc::k_s4_hist, dim3(static_cast<unsigned>(grid)), dim3(256), lds, s, vf, M, FW, F, nblk, ntiles, R,
                       HS, rng, hist, shard_rank, shard_world);
}

// S3 work lists of this rank's mask rows [sh_r0, sh_r1) (all rows when not sharded): a wave per
// mask for the bulk, a workgroup per mask for large masks, largest first.  Rows are split over
// the ranks in contiguous blocks of about equal point counts.
void build_s3_lists(mc_ctx *ctx, const std::vector<int32_t> &frame_start)
{
    const int M = ctx->M, F = ctx->F;
    hipStream_t s = ctx->stream;
    {
        const int64_t tot = ctx->h_off[M];
        const int r = ctx->sh_rank, W = ctx->sh_world;
        auto cut = [&](int k) {  // first row whose cumulative points reach k/W of the total
            if (k <= 0) return 0;
            if (k >= W) return M;
            const int64_t target = (tot * k + W - 1) / W;
            return static_cast<int>(std::lower_bound(ctx->h_off.begin(), ctx->h_off.begin() + M + 1,
                                                     static_cast<int32_t>(target)) - ctx->h_off.begin());
        };
        ctx->sh_r0 = std::min(cut(r), M);
        ctx->sh_r1 = std::max(ctx->sh_r0, std::min(cut(r + 1), M));
    }
    int max_per_frame = 0;
    for (int c = 0; c < F; c++) max_per_frame = std::max(max_per_frame, frame_start[c + 1] - frame_start[c]);
    const bool wave_ok = F <= 64 * mc::kS3wFrameWords64 && max_per_frame < mc::kS3wCounters;
    std::vector<int> small, big;
    for (int g = ctx->sh_r0; g < ctx->sh_r1; g++) {
        const int sz = ctx->h_off[g + 1] - ctx->h_off[g];
        (wave_ok && sz <= mc::kS3SmallPts ? small : big).push_back(g);
    }
    // largest masks first: the long waves start early instead of forming the tail (a stable
    // counting sort by size, descending: std::stable_sort of C3's 81k rows took ~4 ms of host time)
    auto by_size_desc = [&](std::vector<int> &v) {
        if (v.size() < 2) return;
        int mx = 0;
        for (int g : v) mx = std::max(mx, ctx->h_off[g + 1] - ctx->h_off[g]);
        if (mx > (1 << 22)) {
            std::stable_sort(v.begin(), v.end(), [&](int x, int y) {
                return ctx->h_off[x + 1] - ctx->h_off[x] > ctx->h_off[y + 1] - ctx->h_off[y];
            });
            return;
        }
        std::vector<int> start(mx + 2, 0);
        for (int g : v) start[mx - (ctx->h_off[g + 1] - ctx->h_off[g]) + 1]++;
        for (int i = 1; i <= mx + 1; i++) start[i] += start[i - 1];
        std::vector<int> out(v.size());
        for (int g : v) out[start[mx - (ctx->h_off[g + 1] - ctx->h_off[g])]++] = g;
        v.swap(out);
    };
    by_size_desc(small);
    by_size_desc(big);
    ctx->n_s3_small = static_cast<int>(small.size());
    ctx->n_s3_big = static_cast<int>(big.size());
    ctx->d_s3_small.reserve((small.size() + 1) * sizeof(int));
    ctx->d_s3_big.reserve((big.size() + 1) * sizeof(int));
    if (!small.empty())
        MC_HIP(hipMemcpyAsync(ctx->d_s3_small.ptr, small.data(), small.size() * sizeof(int), hipMemcpyHostToDevice, s));
    if (!big.empty())
        MC_HIP(hipMemcpyAsync(ctx->d_s3_big.ptr, big.data(), big.size() * sizeof(int), hipMemcpyHostToDevice, s));
    MC_HIP(hipStreamSynchronize(s));
}

std::vector<int32_t> frame_starts(const mc_ctx *ctx)
{
    std::vector<int32_t> fs(ctx->F + 1, 0);
    int g = 0;
    for (int c = 0; c <= ctx->F; c++) {
        while (g < ctx->M && ctx->h_col[g] < c) g++;
        fs[c] = g;
    }
    return fs;
}

}  // namespace

static void shard_drain_native(mc_ctx *ctx);
static void comm_detach(mc_ctx *ctx);
namespace {
bool sharded(const mc_ctx *ctx);
}

extern "C" {

int mc_ctx_create(int device, mc_ctx **out)
{
    if (!out) return MC_ERR_INVALID;
    *out = nullptr;
    mc_ctx *ctx = new mc_ctx();
    ctx->device = device;
    int rc = guarded(ctx, [&] {
        MC_HIP(hipSetDevice(ctx->device));
        MC_HIP(hipDeviceGetAttribute(&ctx->num_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
        MC_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
        MC_HIP(hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
        MC_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
        MC_HIP(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
        for (int c = 0; c < mc::kBpStreamClasses; c++) {
            MC_HIP(hipStreamCreateWithFlags(&ctx->bp.cls_stream[c], hipStreamNonBlocking));
            MC_HIP(hipEventCreateWithFlags(&ctx->bp.ev_cls[c], hipEventDisableTiming));
        }
        MC_HIP(hipHostMalloc(reinterpret_cast<void **>(&ctx->h_stats), ST_COUNT * sizeof(int), hipHostMallocDefault));
        ctx->d_stats.reserve(ST_COUNT * sizeof(int));
        MC_HIP(hipMemset(ctx->d_stats.ptr, 0, ST_COUNT * sizeof(int)));
    });
    if (rc != MC_OK) {
        mc_ctx_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return MC_OK;
}

void mc_ctx_destroy(mc_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm) {
        try {
            comm_detach(ctx);
        } catch (const McError &) {
        }
    }
    BpState &bp = ctx->bp;
    if (bp.copy) (void)hipStreamSynchronize(bp.copy), (void)hipStreamDestroy(bp.copy);
    if (bp.ev_up) (void)hipEventDestroy(bp.ev_up);
    if (ctx->h_stats) (void)hipHostFree(ctx->h_stats);
    if (bp.h_pack) (void)hipHostFree(bp.h_pack);
    if (bp.h_stat) (void)hipHostFree(bp.h_stat);
    if (bp.ev_pack) (void)hipEventDestroy(bp.ev_pack);
    for (int b = 0; b < 2; b++) {
        if (bp.h_stage[b]) (void)hipHostFree(bp.h_stage[b]);
        if (bp.ev_stage[b]) (void)hipEventDestroy(bp.ev_stage[b]);
    }
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->side) (void)hipStreamSynchronize(ctx->side), (void)hipStreamDestroy(ctx->side);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    for (int c = 0; c < mc::kBpStreamClasses; c++) {
        if (bp.cls_stream[c]) (void)hipStreamSynchronize(bp.cls_stream[c]), (void)hipStreamDestroy(bp.cls_stream[c]);
        if (bp.ev_cls[c]) (void)hipEventDestroy(bp.ev_cls[c]);
    }
    delete ctx;  // every DevBuf frees its memory in its destructor, after the streams above are drained
}

int mc_ctx_set_stream(mc_ctx *ctx, void *hip_stream)
{
    return guarded(ctx, [&] {
        MC_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->own_stream) MC_HIP(hipStreamDestroy(ctx->stream));
        if (hip_stream) {
            ctx->stream = static_cast<hipStream_t>(hip_stream);
            ctx->own_stream = false;
        } else {
            MC_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
            ctx->own_stream = true;
        }
    });
}

void *mc_ctx_get_stream(mc_ctx *ctx) { return ctx ? static_cast<void *>(ctx->stream) : nullptr; }

int mc_ctx_synchronize(mc_ctx *ctx)
{
    return guarded(ctx, [&] {
        MC_HIP(hipStreamSynchronize(ctx->stream));
        ctx->timer.collect();
    });
}

const char *mc_ctx_last_error(mc_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int mc_ctx_set_timing(mc_ctx *ctx, int enable)
{
    return guarded(ctx, [&] {
        MC_HIP(hipStreamSynchronize(ctx->stream));
        ctx->timer.collect();
        ctx->timer.enabled = enable != 0;
    });
}

int mc_ctx_set_timing_filter(mc_ctx *ctx, const char *kernel)
{
    return guarded(ctx, [&] {
        MC_HIP(hipStreamSynchronize(ctx->stream));
        ctx->timer.collect();
        ctx->timer.filter = kernel ? kernel : "";
    });
}

int mc_ctx_get_kernel_time(mc_ctx *ctx, const char *kernel, double *total_ms, int64_t *launches)
{
    return guarded(ctx, [&] {
        MC_HIP(hipStreamSynchronize(ctx->stream));
        ctx->timer.collect();
        auto it = ctx->timer.totals.find(kernel ? kernel : "");
        if (total_ms) *total_ms = it == ctx->timer.totals.end() ? 0.0 : it->second.first;
        if (launches) *launches = it == ctx->timer.totals.end() ? 0 : it->second.second;
    });
}

int mc_ctx_reset_kernel_times(mc_ctx *ctx)
{
    return guarded(ctx, [&] {
        MC_HIP(hipStreamSynchronize(ctx->stream));
        ctx->timer.collect();
        ctx->timer.totals.clear();
    });
}

int mc_ctx_set_memory_budget(mc_ctx *ctx, int64_t bytes)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(bytes >= 0, MC_ERR_INVALID, "negative memory budget");
        ctx->bp.mem_budget = bytes;
    });
}

int mc_debug_counters(mc_ctx *ctx, int64_t *out, int32_t n, int reset)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(out && n >= 1 && n <= 9, MC_ERR_INVALID, "bad counter array");
        MC_HIP(hipDeviceSynchronize());
        unsigned long long c[8] = {};
        MC_HIP(hipMemcpyFromSymbol(c, HIP_SYMBOL(mc::g_bp_dbg), sizeof(c)));
        out[0] = MC_DBG_CHECK ? 1 : 0;
        for (int k = 1; k < n; k++) out[k] = static_cast<int64_t>(c[k - 1]);
        if (reset) {
            const unsigned long long z[8] = {};
            const unsigned zp = 0;
            MC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(mc::g_bp_dbg), z, sizeof(z)));
            MC_HIP(hipMemcpyToSymbol(HIP_SYMBOL(mc::g_bp_dbg_printed), &zp, sizeof(zp)));
        }
    });
}

// ---------------------------------------------------------------------------------------------
// scene input
// ---------------------------------------------------------------------------------------------
__global__ void k_validate_pts(const int *pts, int nnz, int64_t P, int *bad)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nnz; i += gridDim.x * 256)
        if (pts[i] < 0 || pts[i] >= P) atomicOr(bad, 1);
}

int mc_scene_set_masks(mc_ctx *ctx, int64_t num_points, int32_t num_frames, int32_t num_masks_in,
                       const int32_t *mask_col, const int32_t *mask_label, const int64_t *mask_off,
                       const int32_t *mask_pts, int pts_on_device)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(num_points >= 0 && num_points < (int64_t(1) << 31) - 1, MC_ERR_UNSUPPORTED, "num_points out of range");
        MC_REQUIRE(num_frames >= 0 && num_frames <= 16384, MC_ERR_UNSUPPORTED, "num_frames must be <= 16384");
        MC_REQUIRE(num_masks_in >= 0, MC_ERR_INVALID, "num_masks < 0");
        MC_REQUIRE(num_masks_in == 0 || (mask_col && mask_label && mask_off), MC_ERR_INVALID, "null mask arrays");
        MC_REQUIRE(!mask_off || mask_off[0] == 0, MC_ERR_INVALID, "mask_off[0] != 0");
        const int64_t nnz = num_masks_in ? mask_off[num_masks_in] : 0;
        MC_REQUIRE(nnz < (int64_t(1) << 31) - 1, MC_ERR_UNSUPPORTED, "more than 2^31 mask points");
        MC_REQUIRE(nnz == 0 || mask_pts, MC_ERR_INVALID, "null mask_pts");
        ctx->have_scene = ctx->have_graph = ctx->have_nodes = ctx->have_cluster = false;
        ctx->P = num_points;
        ctx->F = num_frames;
        ctx->FW = (num_frames + 63) / 64;
        ctx->M_in = num_masks_in;
        // validation + the frame-skip rule (construction.py:50-51)
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
        {
            std::vector<int> seen(65536, -1);
            for (int g = 0; g < num_masks_in; g++) {
                MC_REQUIRE(seen[mask_label[g]] != mask_col[g], MC_ERR_INVALID, "duplicate mask label within a frame");
                seen[mask_label[g]] = mask_col[g];
            }
        }
        ctx->h_col.clear();
        ctx->h_label.clear();
        ctx->h_in_index.clear();
        ctx->h_off.assign(1, 0);
        for (int g = 0; g < num_masks_in; g++) {
            if (frame_pts[mask_col[g]] == 0) continue;  // masks of a skipped frame have no points
            ctx->h_in_index.push_back(g);
            ctx->h_col.push_back(mask_col[g]);
            ctx->h_label.push_back(mask_label[g]);
            ctx->h_off.push_back(static_cast<int32_t>(mask_off[g + 1]));
        }
        const int M = static_cast<int>(ctx->h_col.size());
        ctx->M = M;
        ctx->nnz = static_cast<int>(nnz);
        MC_REQUIRE(M <= 262144, MC_ERR_UNSUPPORTED, "more than 262144 global masks");
        std::vector<int32_t> frame_start(num_frames + 1, 0);
        {
            int g = 0;
            for (int c = 0; c <= num_frames; c++) {
                while (g < M && ctx->h_col[g] < c) g++;
                frame_start[c] = g;
            }
        }
        const int64_t P = num_points;
        const int F = num_frames, FW = ctx->FW;
        hipStream_t s = ctx->stream;
        ctx->d_mask_off.reserve((M + 1) * sizeof(int));
        ctx->d_mask_col.reserve((M + 1) * sizeof(int));
        ctx->d_mask_label.reserve((M + 1) * sizeof(int));
        ctx->d_frame_start.reserve((F + 2) * sizeof(int));
        ctx->d_mask_pts.reserve((nnz + 1) * sizeof(int));
        ctx->d_valid.reserve(sizeof(int));
        MC_HIP(hipMemcpyAsync(ctx->d_mask_off.ptr, ctx->h_off.data(), (M + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        if (M) {
            MC_HIP(hipMemcpyAsync(ctx->d_mask_col.ptr, ctx->h_col.data(), M * sizeof(int), hipMemcpyHostToDevice, s));
            MC_HIP(hipMemcpyAsync(ctx->d_mask_label.ptr, ctx->h_label.data(), M * sizeof(int), hipMemcpyHostToDevice, s));
        }
        MC_HIP(hipMemcpyAsync(ctx->d_frame_start.ptr, frame_start.data(), (F + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        if (nnz)
            MC_HIP(hipMemcpyAsync(ctx->d_mask_pts.ptr, mask_pts, nnz * sizeof(int),
                                  pts_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        MC_HIP(hipMemsetAsync(ctx->d_valid.ptr, 0, sizeof(int), s));
        if (nnz)
            hipLaunchKernelGGL(k_validate_pts, grid_for(nnz), dim3(256), 0, s, ctx->d_mask_pts.as<int>(),
                               static_cast<int>(nnz), P, ctx->d_valid.as<int>());
        int bad = 0;
        MC_HIP(hipMemcpyAsync(&bad, ctx->d_valid.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
        MC_HIP(hipStreamSynchronize(s));
        MC_REQUIRE(bad == 0, MC_ERR_INVALID, "mask point id out of [0, num_points)");

        // S2/S3/S4 buffers (allocated once per scene; nothing is allocated while building)
        ctx->d_deg.reserve((P + 1) * sizeof(int));
        ctx->d_spread.reserve(mc::kSpread * mc::kSpreadStrideI * sizeof(int));
        MC_HIP(hipMemsetAsync(ctx->d_deg.ptr, 0, (P + 1) * sizeof(int), s));  // kept zero by the S2 scatter
        ctx->d_pt_off.reserve((P + 2) * sizeof(int));
        ctx->d_pt_list.reserve((nnz + 1) * sizeof(unsigned));
        ctx->d_boundary.reserve(P + 1);
        ctx->d_pfm.reserve((P * FW + 1) * sizeof(unsigned long long));
        ctx->d_scan_tmp.reserve((2 * (P / 4096 + 4) + 16) * sizeof(int));
        ctx->d_ctmp.reserve((static_cast<size_t>(M) * F + 1) * sizeof(int));
        ctx->d_crow_len.reserve((M + 1) * sizeof(int));
        ctx->d_useg.reserve(M + 1);
        ctx->d_keep_cnt.reserve((M + 1) * sizeof(int));
        ctx->d_node_flag.reserve((M + 1) * sizeof(int));
        ctx->d_node_pos.reserve((M + 2) * sizeof(int));
        ctx->d_c_off.reserve((M + 2) * sizeof(int));
        ctx->d_c_idx.reserve((static_cast<size_t>(M) * F + 1) * sizeof(int));
        ctx->d_vf.reserve((static_cast<size_t>(M) * FW + 1) * sizeof(unsigned long long));
        ctx->d_hist.reserve((F + 2) * sizeof(unsigned long long));
        ctx->d_s4rng.reserve((M / 64 + 2) * sizeof(int2));
        ctx->d_thr.reserve(32 * sizeof(float));
        ctx->d_isint.reserve(32 * sizeof(int));
        ctx->d_node0_g.reserve((M + 1) * sizeof(int));
        ctx->d_n0_off.reserve((M + 1) * sizeof(int));
        ctx->d_n0_len.reserve((M + 1) * sizeof(int));
        ctx->d_n0_ptoff.reserve((M + 1) * sizeof(int));
        ctx->d_n0_ptlen.reserve((M + 1) * sizeof(int));
        ctx->d_n0_vf.reserve((static_cast<size_t>(M) * FW + 1) * sizeof(unsigned long long));
        ctx->d_owner0.reserve((static_cast<size_t>(M) * F + 1) * sizeof(int));
        ctx->d_node_of_mask.reserve((M + 1) * sizeof(int));
        ctx->d_obj_of_mask.reserve((M + 1) * sizeof(int));
        build_s3_lists(ctx, frame_start);
        ctx->have_scene = true;
    });
}

// ---------------------------------------------------------------------------------------------
// S2–S5
// ---------------------------------------------------------------------------------------------
// S3 undo + S5 + S4 (this rank's tiles of the observer histogram when sharded)
static void graph_build_tail(mc_ctx *ctx)
{
    hipStream_t s = ctx->stream;
    const int F = ctx->F, FW = ctx->FW, M = ctx->M;
    int *stats = ctx->d_stats.as<int>();
    if (M) {  // S3 undo + S5
        TimedScope ts(ctx->timer, s, "s3_undo_s5");
        hipLaunchKernelGGL(mc::k_s3_undo_count, dim3(ceil_div(std::max(M, F + 1), 256)), dim3(256), 0, s,
                           ctx->d_ctmp.as<int>(), ctx->d_crow_len.as<int>(), ctx->d_useg.as<unsigned char>(), M, F,
                           ctx->d_keep_cnt.as<int>(), ctx->d_node_flag.as<int>(),
                           ctx->d_hist.as<unsigned long long>(), ctx->d_spread.as<int>(), stats + ST_NBND);
        mc::scan_device_n(s, ctx->d_keep_cnt.as<int>(), ctx->d_c_off.as<int>(), nullptr, M, stats + ST_NNZC,
                          ctx->d_node_flag.as<int>(), ctx->d_node_pos.as<int>(), stats + ST_N0);
        hipLaunchKernelGGL(mc::k_s3_undo_write, dim3(ceil_div(M, 256)), dim3(256), 0, s, ctx->d_ctmp.as<int>(),
                           ctx->d_crow_len.as<int>(), ctx->d_useg.as<unsigned char>(), ctx->d_mask_col.as<int>(), M,
                           F, FW, ctx->d_c_off.as<int>(), ctx->d_c_idx.as<int>(),
                           ctx->d_vf.as<unsigned long long>());
        hipLaunchKernelGGL(mc::k_s5_nodes, dim3(ceil_div(M, 256)), dim3(256), 0, s, ctx->d_node_pos.as<int>(),
                           ctx->d_useg.as<unsigned char>(), ctx->d_c_off.as<int>(), ctx->d_mask_off.as<int>(),
                           ctx->d_vf.as<unsigned long long>(), M, FW, ctx->d_node0_g.as<int>(),
                           ctx->d_n0_off.as<int>(), ctx->d_n0_len.as<int>(), ctx->d_n0_ptoff.as<int>(),
                           ctx->d_n0_ptlen.as<int>(), ctx->d_n0_vf.as<unsigned long long>(),
                           ctx->d_owner0.as<int>(), ctx->d_node_of_mask.as<int>());
    } else {
        MC_HIP(hipMemsetAsync(ctx->d_hist.ptr, 0, (F + 1) * sizeof(unsigned long long), s));
    }
    {  // S4: observer histogram (the thresholds follow in graph_build_thresholds)
        TimedScope ts(ctx->timer, s, "s4_observer_hist");
        launch_hist(s, ctx->d_vf.as<unsigned long long>(), M, F, ctx->d_hist.as<unsigned long long>(),
                    ctx->d_s4rng.as<int2>(), ctx->sh_rank, ctx->sh_world);
    }
    MC_HIP(hipGetLastError());
}

static void graph_build_thresholds(mc_ctx *ctx)
{
    hipStream_t s = ctx->stream;
    const int F = ctx->F;
    int *stats = ctx->d_stats.as<int>();
    {
        TimedScope ts(ctx->timer, s, "s4_observer_hist");
        hipLaunchKernelGGL(mc::k_s4_thresholds, dim3(1), dim3(256), (F + 1) * sizeof(unsigned long long), s,
                           ctx->d_hist.as<unsigned long long>(), F, ctx->d_thr.as<float>(), ctx->d_isint.as<int>(),
                           stats + ST_NTHR, stats + ST_THR_STATUS);
    }
    MC_HIP(hipGetLastError());
    // level-0 nodes live in the graph's buffers
    ctx->n0_pool = ctx->d_c_idx.as<int>();
    ctx->n0_pts = ctx->d_mask_pts.as<int>();
    ctx->Mn = ctx->M;
    ctx->n0_pts_total = ctx->nnz;
    ctx->nodes_from_graph = true;
    ctx->have_graph = true;
    ctx->have_nodes = true;
}

int mc_graph_build(mc_ctx *ctx, const mc_graph_params *params)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_scene, MC_ERR_STATE, "mc_graph_build before mc_scene_set_masks");
        MC_REQUIRE(params, MC_ERR_INVALID, "null params");
        hipStream_t s = ctx->stream;
        const int64_t P = ctx->P;
        const int F = ctx->F, FW = ctx->FW, M = ctx->M, nnz = ctx->nnz;
        int *stats = ctx->d_stats.as<int>();
        ctx->have_cluster = false;
        ctx->have_graph = ctx->have_nodes = false;
        ctx->sh_pending = 0;
        ctx->sh_params = *params;
        {  // S2
            TimedScope ts(ctx->timer, s, "s2_point_lists");
            hipLaunchKernelGGL(mc::k_s2_degree, grid_for(nnz), dim3(256), 0, s, ctx->d_mask_pts.as<int>(), nnz,
                               ctx->d_deg.as<int>(), stats, static_cast<int>(ST_COUNT), ctx->d_spread.as<int>());
            mc::scan_large(s, ctx->d_deg.as<int>(), ctx->d_pt_off.as<int>(), static_cast<int>(P), ctx->d_scan_tmp.as<int>());
            if (M)
                hipLaunchKernelGGL(mc::k_s2_scatter, dim3(M), dim3(256), 0, s, ctx->d_mask_off.as<int>(),
                                   ctx->d_mask_pts.as<int>(), ctx->d_mask_col.as<int>(), ctx->d_frame_start.as<int>(),
                                   ctx->d_pt_off.as<int>(), ctx->d_deg.as<int>(), ctx->d_pt_list.as<unsigned>());
            if (P)
                hipLaunchKernelGGL(mc::k_s2_points, dim3(ceil_div(P, 256)), dim3(256), 0, s, ctx->d_pt_off.as<int>(),
                                   ctx->d_pt_list.as<unsigned>(), static_cast<int>(P), FW,
                                   ctx->d_boundary.as<unsigned char>(), ctx->d_pfm.as<unsigned long long>(),
                                   ctx->d_spread.as<int>());
        }
        if (M) {  // S3
            TimedScope ts(ctx->timer, s, "s3_masks");
            // large masks (workgroup per mask) on the side stream, concurrent with the wave kernel
            const bool fork = ctx->n_s3_big && ctx->n_s3_small;
            if (fork) {
                MC_HIP(hipEventRecord(ctx->ev_fork, s));
                MC_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
            }
            if (ctx->n_s3_big)
                hipLaunchKernelGGL(mc::k_s3_masks<mc::kS3BigW>, grid_for(ctx->n_s3_big, 1, 8192),
                                   dim3(mc::S3Cfg<mc::kS3BigW>::NT), 0,
                                   fork ? ctx->side : s,
                                   ctx->d_s3_big.as<int>(), ctx->n_s3_big, ctx->d_mask_off.as<int>(),
                                   ctx->d_mask_pts.as<int>(), ctx->d_pt_off.as<int>(), ctx->d_pt_list.as<unsigned>(),
                                   ctx->d_boundary.as<unsigned char>(), ctx->d_pfm.as<unsigned long long>(), FW,
                                   ctx->d_frame_start.as<int>(), ctx->d_mask_label.as<int>(), F,
                                   params->mask_visible_threshold, params->contained_threshold,
                                   params->undersegment_filter_threshold, ctx->d_ctmp.as<int>(),
                                   ctx->d_crow_len.as<int>(), ctx->d_useg.as<unsigned char>());
            if (ctx->n_s3_small)
                hipLaunchKernelGGL(mc::k_s3_masks<1>, grid_for(ctx->n_s3_small, 4, 16384), dim3(256), 0, s,
                                   ctx->d_s3_small.as<int>(), ctx->n_s3_small, ctx->d_mask_off.as<int>(),
                                   ctx->d_mask_pts.as<int>(), ctx->d_pt_off.as<int>(), ctx->d_pt_list.as<unsigned>(),
                                   ctx->d_boundary.as<unsigned char>(), ctx->d_pfm.as<unsigned long long>(), FW,
                                   ctx->d_frame_start.as<int>(), ctx->d_mask_label.as<int>(), F,
                                   params->mask_visible_threshold, params->contained_threshold,
                                   params->undersegment_filter_threshold, ctx->d_ctmp.as<int>(),
                                   ctx->d_crow_len.as<int>(), ctx->d_useg.as<unsigned char>());
            if (fork) {
                MC_HIP(hipEventRecord(ctx->ev_join, ctx->side));
                MC_HIP(hipStreamWaitEvent(s, ctx->ev_join, 0));
            }
        }
        if (sharded(ctx)) {  // this rank's S3 rows go to the others first (mc_shard_export/import)
            ctx->sh_pending = MC_SHARD_S3;
            ctx->sh_s3_words = -1;
            if (ctx->comm) shard_drain_native(ctx);  // S3 rows, then the histogram, over RCCL
            return;
        }
        graph_build_tail(ctx);
        graph_build_thresholds(ctx);
    });
}

int mc_graph_get_info(mc_ctx *ctx, mc_graph_info *info)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_graph && info, MC_ERR_STATE, "no graph");
        sync_stats(ctx);
        const int *h = ctx->h_stats;
        info->num_points = ctx->P;
        info->num_frames = ctx->F;
        info->num_masks = ctx->M;
        info->num_nodes0 = h[ST_N0];
        info->num_undersegment = ctx->M - h[ST_N0];
        info->num_contained = h[ST_NNZC];
        info->num_boundary = h[ST_NBND];
        info->num_thresholds = h[ST_NTHR];
        info->threshold_status = h[ST_THR_STATUS];
    });
}

int mc_graph_get_global_masks(mc_ctx *ctx, int32_t *input_index)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_scene, MC_ERR_STATE, "no scene");
        std::copy(ctx->h_in_index.begin(), ctx->h_in_index.end(), input_index);
    });
}

int mc_graph_get_boundary(mc_ctx *ctx, uint8_t *flags)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_graph, MC_ERR_STATE, "no graph");
        if (ctx->P) MC_HIP(hipMemcpyAsync(flags, ctx->d_boundary.ptr, ctx->P, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int mc_graph_get_point_in_mask(mc_ctx *ctx, uint16_t *pim)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_graph, MC_ERR_STATE, "no graph");
        const size_t bytes = static_cast<size_t>(ctx->P) * ctx->F * sizeof(uint16_t);
        if (!bytes) return;
        DevBuf tmp;
        tmp.reserve(bytes);
        MC_HIP(hipMemsetAsync(tmp.ptr, 0, bytes, ctx->stream));
        hipLaunchKernelGGL(mc::k_s2_dense_pim, dim3(ceil_div(ctx->P, 256)), dim3(256), 0, ctx->stream,
                           ctx->d_pt_off.as<int>(), ctx->d_pt_list.as<unsigned>(), ctx->d_mask_label.as<int>(),
                           ctx->d_frame_start.as<int>(), static_cast<int>(ctx->P), ctx->F, tmp.as<unsigned short>());
        MC_HIP(hipMemcpyAsync(pim, tmp.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
        tmp.release();
    });
}

int mc_graph_get_point_frame_bits(mc_ctx *ctx, uint64_t *bits)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_graph, MC_ERR_STATE, "no graph");
        const size_t bytes = static_cast<size_t>(ctx->P) * ctx->FW * 8;
        if (bytes) MC_HIP(hipMemcpyAsync(bits, ctx->d_pfm.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int mc_graph_get_visible_frame_bits(mc_ctx *ctx, uint64_t *bits)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_graph, MC_ERR_STATE, "no graph");
        const size_t bytes = static_cast<size_t>(ctx->M) * ctx->FW * 8;
        if (bytes) MC_HIP(hipMemcpyAsync(bits, ctx->d_vf.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int mc_graph_get_contained(mc_ctx *ctx, int64_t *row_off, int32_t *col_idx)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_graph, MC_ERR_STATE, "no graph");
        sync_stats(ctx);
        std::vector<int32_t> off(ctx->M + 1);
        MC_HIP(hipMemcpyAsync(off.data(), ctx->d_c_off.ptr, (ctx->M + 1) * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        const int nnzc = ctx->h_stats[ST_NNZC];
        if (nnzc) MC_HIP(hipMemcpyAsync(col_idx, ctx->d_c_idx.ptr, nnzc * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i <= ctx->M; i++) row_off[i] = ctx->M ? off[i] : 0;
    });
}

int mc_graph_get_undersegment(mc_ctx *ctx, int32_t *ids)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_graph, MC_ERR_STATE, "no graph");
        std::vector<uint8_t> u(ctx->M);
        if (ctx->M) MC_HIP(hipMemcpyAsync(u.data(), ctx->d_useg.ptr, ctx->M, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
        int k = 0;
        for (int g = 0; g < ctx->M; g++)
            if (u[g]) ids[k++] = g;
    });
}

int mc_graph_get_nodes0(mc_ctx *ctx, int32_t *mask_index)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_graph, MC_ERR_STATE, "no graph");
        sync_stats(ctx);
        const int n0 = ctx->h_stats[ST_N0];
        if (n0) MC_HIP(hipMemcpyAsync(mask_index, ctx->d_node0_g.ptr, n0 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int mc_graph_get_observer_hist(mc_ctx *ctx, uint64_t *hist)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_graph, MC_ERR_STATE, "no graph");
        MC_HIP(hipMemcpyAsync(hist, ctx->d_hist.ptr, (ctx->F + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int mc_graph_get_thresholds(mc_ctx *ctx, float *thr, int32_t *is_int, int32_t *n)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_graph, MC_ERR_STATE, "no graph");
        sync_stats(ctx);
        MC_HIP(hipMemcpyAsync(thr, ctx->d_thr.ptr, mc::kMaxThresholds * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipMemcpyAsync(is_int, ctx->d_isint.ptr, mc::kMaxThresholds * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
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
        hipLaunchKernelGGL(mc::k_s4_thresholds, dim3(1), dim3(256), (F + 1) * sizeof(unsigned long long), s,
                           hist.as<unsigned long long>(), F,
                           dthr.as<float>(), disint.as<int>(), st.as<int>(), st.as<int>() + 1);
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
        ctx->have_graph = false;
        ctx->have_cluster = false;
        ctx->nodes_from_graph = false;
        ctx->F = num_frames;
        ctx->FW = (num_frames + 63) / 64;
        ctx->P = num_points;
        ctx->Mn = num_masks;
        ctx->N0 = num_nodes;
        ctx->nnzC0 = nc;
        ctx->n0_pts_total = np;
        const int n = num_nodes, FW = ctx->FW;
        ctx->d_n0_off.reserve((n + 1) * sizeof(int));
        ctx->d_n0_len.reserve((n + 1) * sizeof(int));
        ctx->d_n0_ptoff.reserve((n + 1) * sizeof(int));
        ctx->d_n0_ptlen.reserve((n + 1) * sizeof(int));
        ctx->d_n0_vf.reserve((static_cast<size_t>(n) * FW + 1) * 8);
        ctx->d_user_cidx.reserve((nc + 1) * sizeof(int));
        ctx->d_user_pts.reserve((np + 1) * sizeof(int));
        ctx->d_owner0.reserve((nc + 1) * sizeof(int));
        DevBuf t1, t2;
        t1.reserve((n + 1) * 8);
        t2.reserve((n + 1) * 8);
        if (n) {
            MC_HIP(hipMemcpyAsync(t1.ptr, c_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
            MC_HIP(hipMemcpyAsync(t2.ptr, pt_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
            if (FW) MC_HIP(hipMemcpyAsync(ctx->d_n0_vf.ptr, vf_bits, static_cast<size_t>(n) * FW * 8, hipMemcpyHostToDevice, s));
            if (nc) MC_HIP(hipMemcpyAsync(ctx->d_user_cidx.ptr, c_idx, nc * sizeof(int), hipMemcpyHostToDevice, s));
            if (np) MC_HIP(hipMemcpyAsync(ctx->d_user_pts.ptr, pt_idx, np * sizeof(int), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_nodes_from_csr, grid_for(n), dim3(256), 0, s, n, t1.as<int64_t>(), t2.as<int64_t>(),
                               ctx->d_n0_off.as<int>(), ctx->d_n0_len.as<int>(), ctx->d_n0_ptoff.as<int>(),
                               ctx->d_n0_ptlen.as<int>(), ctx->d_owner0.as<int>());
        }
        MC_HIP(hipStreamSynchronize(s));
        t1.release();
        t2.release();
        ctx->n0_pool = ctx->d_user_cidx.as<int>();
        ctx->n0_pts = ctx->d_user_pts.as<int>();
        ctx->have_nodes = true;
    });
}

// ---------------------------------------------------------------------------------------------
// S6
// ---------------------------------------------------------------------------------------------
static mc::EdgeCap edge_cap(mc_ctx *ctx)
{
    if (ctx->cap_edges <= 0) return mc::EdgeCap{nullptr, nullptr, 0};
    return mc::EdgeCap{ctx->d_cap_buf.as<unsigned long long>(), ctx->d_cap_cnt.as<unsigned long long>(),
                       static_cast<long long>(ctx->cap_edges)};
}

// S6 iterations t_begin .. nthr-1 (after_pairs: iteration t_begin's pairs are done) and the final
// object state; the level-t node arrays are re-derived from the ping-pong pools
static void s6_iterations(mc_ctx *ctx, int t_begin, bool after_pairs)
{
    hipStream_t s = ctx->stream;
    const int nthr = ctx->s6_nthr, N0 = ctx->N0, FW = ctx->FW, Mn = ctx->Mn;
    const bool dense_obs = ctx->s6_dense_obs;
    const float ctf = ctx->s6_ctf;
    const size_t n0 = static_cast<size_t>(std::max(N0, 1));
    int *Nlev = ctx->d_Nlev.as<int>();
    int *dcap = ctx->d_cap.as<int>();
    MC_REQUIRE(t_begin == 0, MC_ERR_STATE, "S6 resumes only at iteration 0");
    const int *cur_off = ctx->d_n0_off.as<int>(), *cur_len = ctx->d_n0_len.as<int>(), *cur_pool = ctx->n0_pool;
    const unsigned long long *cur_vf = ctx->d_n0_vf.as<unsigned long long>();
    const dim3 gN = grid_for(N0), gW = grid_for(N0, mc::kPairWaves, 2048), gK = grid_for(N0, 1, 2048);
    for (int t = t_begin; t < nthr; t++) {
        const int *dN = Nlev + t;
        int *dNn = Nlev + t + 1;
        const bool toA = (t % 2) == 0;
        int *nx_off = toA ? ctx->d_offA.as<int>() : ctx->d_offB.as<int>();
        int *nx_len = toA ? ctx->d_lenA.as<int>() : ctx->d_lenB.as<int>();
        int *nx_pool = toA ? ctx->d_poolA.as<int>() : ctx->d_poolB.as<int>();
        int *nx_own = toA ? ctx->d_ownA.as<int>() : ctx->d_ownB.as<int>();
        unsigned long long *nx_vf = toA ? ctx->d_vfA.as<unsigned long long>() : ctx->d_vfB.as<unsigned long long>();
        if (t == t_begin && after_pairs) {
            // level 0's pairs ran on every rank's share and their forests were united
        } else if (!dense_obs) {
            TimedScope ts(ctx->timer, s, "s6_pairs");
            const mc::OvfWork ow{ctx->d_scratch.as<int>(), ctx->d_touched.as<int>(), N0, ctx->d_ovf_n.as<int>() + 1};
            hipLaunchKernelGGL(mc::k6_pairs, gW, dim3(256), 0, s, dN, cur_off, cur_len, cur_pool,
                               ctx->d_coloff.as<int>(), ctx->d_collen.as<int>(), ctx->d_colnodes.as<int>(), cur_vf, FW,
                               ctx->d_thr.as<float>(), t, ctf, ctx->d_parent.as<int>(),
                               ctx->d_edges.as<unsigned long long>(), ow, 0, 1, edge_cap(ctx));
        } else {
            TimedScope ts(ctx->timer, s, "s6_pairs");
            hipLaunchKernelGGL(mc::k6_parent_init, gN, dim3(256), 0, s, dN, ctx->d_parent.as<int>());
            hipLaunchKernelGGL(mc::k6_pairs_dense, dim3(4096), dim3(256), 0, s, dN, cur_vf, FW,
                               ctx->d_thr.as<float>(), t, ctx->d_parent.as<int>(),
                               ctx->d_edges.as<unsigned long long>(), edge_cap(ctx));
        }
        {
            TimedScope ts(ctx->timer, s, "s6_components");
            if (t > 0 && N0 <= kFusedComponentsMaxN0) {  // N_t <= N_1, typically N0 / 8: one workgroup
                hipLaunchKernelGGL(mc::k6_components, dim3(1), dim3(1024), 0, s, dN, dNn, ctx->d_parent.as<int>(),
                                   ctx->d_root.as<int>(), ctx->d_rank.as<int>(), cur_len, ctx->d_label.as<int>(),
                                   ctx->d_levels.as<int>() + static_cast<size_t>(t) * n0, ctx->d_memcnt.as<int>(),
                                   ctx->d_memoff.as<int>(), ctx->d_ublen.as<int>(), ctx->d_newoff.as<int>(),
                                   dcap + t + 1, ctx->d_members.as<int>(), ctx->d_ovf_n.as<int>());
            } else {
                hipLaunchKernelGGL(mc::k6_compress, gN, dim3(256), 0, s, dN, ctx->d_parent.as<int>(),
                                   ctx->d_root.as<int>(), ctx->d_isroot.as<int>(), ctx->d_ublen.as<int>(),
                                   ctx->d_ovf_n.as<int>());
                mc::scan_device_n(s, ctx->d_isroot.as<int>(), ctx->d_rank.as<int>(), dN, 0, dNn);
                hipLaunchKernelGGL(mc::k6_relabel, gN, dim3(256), 0, s, dN, ctx->d_root.as<int>(),
                                   ctx->d_rank.as<int>(), cur_len, ctx->d_label.as<int>(),
                                   ctx->d_levels.as<int>() + static_cast<size_t>(t) * n0, ctx->d_memcnt.as<int>(),
                                   ctx->d_ublen.as<int>());
                mc::scan_device_n(s, ctx->d_memcnt.as<int>(), ctx->d_memoff.as<int>(), dNn, 0, nullptr,
                                  ctx->d_ublen.as<int>(), ctx->d_newoff.as<int>(), dcap + t + 1);
                hipLaunchKernelGGL(mc::k6_memscatter, gN, dim3(256), 0, s, dN, 0, ctx->d_label.as<int>(),
                                   ctx->d_memoff.as<int>(), ctx->d_memcnt.as<int>(), ctx->d_members.as<int>(),
                                   nullptr);
            }
        }
        {
            TimedScope ts(ctx->timer, s, "s6_merge");
            // + the next iteration's column lists (nodes containing each mask, relabelled)
            const bool cols = !dense_obs && t + 1 < nthr;
            const mc::ColUpdate cu{Mn, dNn, ctx->d_coloff.as<int>(), ctx->d_collen.as<int>(),
                                   ctx->d_colnodes.as<int>(), cols ? ctx->d_label.as<int>() : nullptr,
                                   ctx->d_parent.as<int>(), N0, ctx->d_label.as<int>(),
                                   ctx->d_final_label.as<int>()};
            hipLaunchKernelGGL(mc::k6_merge, gK, dim3(256), 0, s, dNn, ctx->d_memoff.as<int>(),
                               ctx->d_members.as<int>(), cur_off, cur_len, cur_pool, cur_vf, FW,
                               ctx->d_newoff.as<int>(), nx_off, nx_len, nx_pool, nx_own, nx_vf, cu);
        }
        cur_off = nx_off;
        cur_len = nx_len;
        cur_pool = nx_pool;
        cur_vf = nx_vf;
    }
    ctx->fin_off = cur_off;
    ctx->fin_len = cur_len;
    ctx->fin_pool = cur_pool;
    ctx->fin_vf = cur_vf;
    ctx->n_iter = nthr;
    // ---- final point sets (node.py:35), per-object range bitmaps ----
    const int *dK = Nlev + nthr;
    int *stats = ctx->d_stats.as<int>();
    const bool point_path = ctx->nodes_from_graph;
    {
        TimedScope ts(ctx->timer, s, "s7_points");
        hipLaunchKernelGGL(mc::k7_reset, gN, dim3(256), 0, s, N0, ctx->d_pmin.as<int>(), ctx->d_pmax.as<int>());
        if (point_path) {
            hipLaunchKernelGGL(mc::k7_obj_of_mask, grid_for(ctx->M), dim3(256), 0, s, ctx->M,
                               ctx->d_node_of_mask.as<int>(), ctx->d_final_label.as<int>(),
                               ctx->d_obj_of_mask.as<int>());
            hipLaunchKernelGGL(mc::k7p_points<0>, dim3(ceil_div(ctx->P, 256)), dim3(256), 0, s, static_cast<int>(ctx->P),
                               ctx->d_pt_off.as<int>(), ctx->d_pt_list.as<unsigned>(), ctx->d_frame_start.as<int>(),
                               ctx->d_obj_of_mask.as<int>(), ctx->d_pmin.as<int>(), ctx->d_pmax.as<int>(), nullptr,
                               nullptr, stats + ST_OBJOVF);
        }
        else
            hipLaunchKernelGGL(mc::k7_minmax, gW, dim3(256), 0, s, N0, ctx->d_final_label.as<int>(),
                               ctx->d_n0_ptoff.as<int>(), ctx->d_n0_ptlen.as<int>(), ctx->n0_pts,
                               ctx->d_pmin.as<int>(), ctx->d_pmax.as<int>());
        hipLaunchKernelGGL(mc::k7_words, gN, dim3(256), 0, s, dK, ctx->d_pmin.as<int>(), ctx->d_pmax.as<int>(),
                           ctx->d_nwords.as<int>(), stats + ST_K);
        mc::scan_device_n(s, ctx->d_nwords.as<int>(), ctx->d_woff.as<int>(), dK, 0, stats + ST_WORDS);
    }
    sync_stats(ctx);  // bitmap capacity
    ctx->K = ctx->h_stats[ST_K];
    const bool use_points = point_path && ctx->h_stats[ST_OBJOVF] == 0;
    if (point_path && !use_points) {  // a point in > 8 objects: redo the ranges per node
        hipLaunchKernelGGL(mc::k7_reset, gN, dim3(256), 0, s, N0, ctx->d_pmin.as<int>(), ctx->d_pmax.as<int>());
        hipLaunchKernelGGL(mc::k7_minmax, gW, dim3(256), 0, s, N0, ctx->d_final_label.as<int>(),
                           ctx->d_n0_ptoff.as<int>(), ctx->d_n0_ptlen.as<int>(), ctx->n0_pts,
                           ctx->d_pmin.as<int>(), ctx->d_pmax.as<int>());
        hipLaunchKernelGGL(mc::k7_words, gN, dim3(256), 0, s, dK, ctx->d_pmin.as<int>(), ctx->d_pmax.as<int>(),
                           ctx->d_nwords.as<int>(), stats + ST_K);
        mc::scan_device_n(s, ctx->d_nwords.as<int>(), ctx->d_woff.as<int>(), dK, 0, stats + ST_WORDS);
        sync_stats(ctx);
    }
    const size_t words = static_cast<size_t>(std::max(ctx->h_stats[ST_WORDS], 1));
    ctx->d_bm.reserve(words * 8);
    {
        TimedScope ts(ctx->timer, s, "s7_points");
        MC_HIP(hipMemsetAsync(ctx->d_bm.ptr, 0, words * 8, s));
        if (use_points)
            hipLaunchKernelGGL(mc::k7p_points<1>, dim3(ceil_div(ctx->P, 256)), dim3(256), 0, s, static_cast<int>(ctx->P),
                               ctx->d_pt_off.as<int>(), ctx->d_pt_list.as<unsigned>(), ctx->d_frame_start.as<int>(),
                               ctx->d_obj_of_mask.as<int>(), ctx->d_pmin.as<int>(), ctx->d_pmax.as<int>(),
                               ctx->d_woff.as<int>(), ctx->d_bm.as<unsigned long long>(), stats + ST_OBJOVF);
        else
            hipLaunchKernelGGL(mc::k7_setbits, gW, dim3(256), 0, s, N0, ctx->d_final_label.as<int>(),
                               ctx->d_n0_ptoff.as<int>(), ctx->d_n0_ptlen.as<int>(), ctx->n0_pts,
                               ctx->d_pmin.as<int>(), ctx->d_woff.as<int>(), ctx->d_bm.as<unsigned long long>());
        hipLaunchKernelGGL(mc::k7_count, gK, dim3(256), 0, s, dK, ctx->d_woff.as<int>(),
                           ctx->d_bm.as<unsigned long long>(), ctx->d_ptcnt.as<int>());
        mc::scan_device_n(s, ctx->d_ptcnt.as<int>(), ctx->d_ptoff_out.as<int>(), dK, 0, stats + ST_NPTS);
        hipLaunchKernelGGL(mc::k7_extract, gK, dim3(256), 0, s, dK, ctx->d_woff.as<int>(),
                           ctx->d_bm.as<unsigned long long>(), ctx->d_pmin.as<int>(), ctx->d_ptoff_out.as<int>(),
                           ctx->d_pts_out.as<int>());
    }
    MC_HIP(hipGetLastError());
    MC_HIP(hipMemcpyAsync(ctx->h_stats, ctx->d_stats.ptr, ST_COUNT * sizeof(int), hipMemcpyDeviceToHost, s));
    ctx->have_cluster = true;
}

int mc_cluster_run(mc_ctx *ctx, const float *thresholds, int32_t n, double connect_threshold)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_nodes, MC_ERR_STATE, "mc_cluster_run before mc_graph_build / mc_nodes_set");
        // (edge capture on a sharded context: iteration 0 evaluates only this rank's pair rows, so its
        // capture holds those rows' edges and the driver gathers them, graph_shard.ShardedGraph.edges;
        // the later iterations run replicated and every rank captures all of their edges)
        hipStream_t s = ctx->stream;
        int *stats = ctx->d_stats.as<int>();
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
        const int N0 = ctx->N0, FW = ctx->FW, Mn = ctx->Mn;
        MC_REQUIRE(!(N0 == 0 && nthr > 0), MC_ERR_NO_NODES, "no nodes to cluster (torch.stack of an empty list)");
        const bool dense = !(connect_threshold > 0.0);  // ct <= 0: all pairs with O >= thr (NaN: no edge)
        const bool ct_nan = std::isnan(connect_threshold);
        const bool dense_obs = dense && !ct_nan;
        const float ctf = static_cast<float>(connect_threshold);  // torch compares in float32
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

        int *Nlev = ctx->d_Nlev.as<int>();
        int *dcap = ctx->d_cap.as<int>();
        hipLaunchKernelGGL(mc::k6_init, grid_for(std::max<int64_t>(N0, nthr)), dim3(256), 0, s, N0,
                           ctx->d_final_label.as<int>(), ctx->nodes_from_graph ? stats + ST_N0 : nullptr, N0, Nlev,
                           dcap, ctx->nodes_from_graph ? stats + ST_NNZC : nullptr, static_cast<int>(ctx->nnzC0),
                           ctx->d_edges.as<unsigned long long>(), nthr);

        if (ctx->cap_edges > 0) {
            ctx->d_cap_buf.reserve(static_cast<size_t>(ctx->cap_edges) * 8);
            ctx->d_cap_cnt.reserve(8);
            MC_HIP(hipMemsetAsync(ctx->d_cap_cnt.ptr, 0, 8, s));
        }
        const dim3 gE = grid_for(std::max<int64_t>(N0, ctx->nnzC0)), gC = grid_for(std::max(N0, Mn), 64, 8192);
        const int *cur_pool = ctx->n0_pool, *cur_own = ctx->d_owner0.as<int>();
        if (!dense_obs && nthr > 0) {  // level-0 column lists (nodes contained by each mask)
            TimedScope ts(ctx->timer, s, "s6_columns");
            hipLaunchKernelGGL(mc::k6_colcount, gE, dim3(256), 0, s, Nlev, dcap, cur_pool, cur_own,
                               ctx->d_parent.as<int>(), ctx->d_colcnt.as<int>());
            mc::scan_device_n(s, ctx->d_colcnt.as<int>(), ctx->d_coloff.as<int>(), nullptr, Mn, nullptr);
            hipLaunchKernelGGL(mc::k6_colscatter, gE, dim3(256), 0, s, dcap, cur_pool, cur_own,
                               ctx->d_coloff.as<int>(), ctx->d_colcnt.as<int>(), ctx->d_colnodes.as<int>());
            hipLaunchKernelGGL(mc::k6_colupdate, gC, dim3(64), 0, s, Mn, Nlev, ctx->d_coloff.as<int>(),
                               ctx->d_collen.as<int>(), ctx->d_colnodes.as<int>(), nullptr, ctx->d_parent.as<int>());
        }
        ctx->s6_nthr = nthr;
        ctx->s6_dense_obs = dense_obs;
        ctx->s6_ctf = ctf;
        ctx->have_cluster = false;
        ctx->sh_pending = 0;
        if (nthr > 0 && N0 > 0 && sharded(ctx) && !dense_obs) {
            // iteration 0 (the N0 x N0 pairs) on this rank's rows; the union-find forests of all
            // ranks are united by mc_shard_import(MC_SHARD_FOREST), which runs the rest
            TimedScope ts(ctx->timer, s, "s6_pairs");
            const mc::OvfWork ow{ctx->d_scratch.as<int>(), ctx->d_touched.as<int>(), N0, ctx->d_ovf_n.as<int>() + 1};
            hipLaunchKernelGGL(mc::k6_pairs, grid_for(N0, mc::kPairWaves, 2048), dim3(256), 0, s, Nlev,
                               ctx->d_n0_off.as<int>(), ctx->d_n0_len.as<int>(), ctx->n0_pool, ctx->d_coloff.as<int>(),
                               ctx->d_collen.as<int>(), ctx->d_colnodes.as<int>(), ctx->d_n0_vf.as<unsigned long long>(),
                               FW, ctx->d_thr.as<float>(), 0, ctf, ctx->d_parent.as<int>(),
                               ctx->d_edges.as<unsigned long long>(), ow, ctx->sh_rank, ctx->sh_world,
                               mc::EdgeCap{nullptr, nullptr, 0});
            MC_HIP(hipGetLastError());
            ctx->sh_pending = MC_SHARD_FOREST;
            if (ctx->comm) shard_drain_native(ctx);  // the forests over RCCL, then the rest of S6
            return;
        }
        s6_iterations(ctx, 0, false);
    });
}

// ---------------------------------------------------------------------------------------------
// row-block sharding over processes; kernels in mc_shard_kernels.inl
// ---------------------------------------------------------------------------------------------
int mc_shard_set(mc_ctx *ctx, int32_t rank, int32_t world)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(world >= 1 && world <= 1024 && rank >= 0 && rank < world, MC_ERR_INVALID, "bad rank / world");
        MC_REQUIRE(!ctx->comm, MC_ERR_STATE, "a communicator is attached (rank / world come from it; detach first)");
        ctx->sh_rank = rank;
        ctx->sh_world = world;
        ctx->sh_pending = 0;
        if (ctx->have_scene) build_s3_lists(ctx, frame_starts(ctx));
    });
}

int mc_shard_pending(mc_ctx *ctx, int32_t *phase)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(phase, MC_ERR_INVALID, "null phase");
        *phase = ctx->sh_pending;
    });
}

static void shard_export(mc_ctx *ctx, int32_t phase, void *dst_dev, int64_t *bytes)
{
    {
        MC_REQUIRE(bytes, MC_ERR_INVALID, "null bytes");
        MC_REQUIRE(phase == ctx->sh_pending && phase != 0, MC_ERR_STATE, "no such exchange pending");
        hipStream_t s = ctx->stream;
        if (phase == MC_SHARD_S3) {
            const int nr = ctx->sh_r1 - ctx->sh_r0;
            if (ctx->sh_s3_words < 0) {  // entry offsets of this rank's rows + their total (one host sync)
                ctx->d_sh_eoff.reserve((nr + 2) * 4);
                DevBuf dt;
                dt.reserve(8);
                mc::scan_device_n(s, ctx->d_crow_len.as<int>() + ctx->sh_r0, ctx->d_sh_eoff.as<int>(), nullptr, nr,
                                  dt.as<int>());
                int h = 0;
                MC_HIP(hipMemcpyAsync(&h, dt.ptr, 4, hipMemcpyDeviceToHost, s));
                MC_HIP(hipStreamSynchronize(s));
                ctx->sh_s3_words = 2 + 2 * static_cast<int64_t>(nr) + h;
            }
            *bytes = 4 * ctx->sh_s3_words;
            if (dst_dev)
                hipLaunchKernelGGL(mc::k_sh_s3_pack, grid_for(std::max(nr, 1) * 64, 256, 2048), dim3(256), 0, s,
                                   ctx->sh_r0, ctx->sh_r1, ctx->F, ctx->d_ctmp.as<int>(), ctx->d_crow_len.as<int>(),
                                   ctx->d_useg.as<unsigned char>(), ctx->d_sh_eoff.as<int>(), static_cast<int *>(dst_dev));
        } else if (phase == MC_SHARD_HIST) {
            *bytes = 8 * static_cast<int64_t>(ctx->F + 1);
            if (dst_dev)
                MC_HIP(hipMemcpyAsync(dst_dev, ctx->d_hist.ptr, *bytes, hipMemcpyDeviceToDevice, s));
        } else if (phase == MC_SHARD_FOREST) {
            *bytes = 4 * (static_cast<int64_t>(ctx->N0) + 2);
            if (dst_dev)
                hipLaunchKernelGGL(mc::k_sh_forest_export, grid_for(ctx->N0), dim3(256), 0, s, ctx->d_Nlev.as<int>(),
                                   ctx->d_parent.as<int>(), ctx->d_edges.as<unsigned long long>(),
                                   static_cast<int *>(dst_dev), ctx->N0);
        } else {
            throw McError{MC_ERR_INVALID, "unknown exchange phase"};
        }
        MC_HIP(hipGetLastError());
    }
}

static void shard_import(mc_ctx *ctx, int32_t phase, const void *src_dev, int64_t stride_bytes)
{
    {
        MC_REQUIRE(phase == ctx->sh_pending && phase != 0, MC_ERR_STATE, "no such exchange pending");
        MC_REQUIRE(src_dev, MC_ERR_INVALID, "null source");
        hipStream_t s = ctx->stream;
        const int W = ctx->sh_world;
        if (phase == MC_SHARD_S3) {
            MC_REQUIRE(stride_bytes % 4 == 0 && stride_bytes >= 8, MC_ERR_INVALID, "bad S3 block stride");
            hipLaunchKernelGGL(mc::k_sh_s3_unpack, dim3(mc::kUnpackWg, W), dim3(256), 0, s,
                               static_cast<const int *>(src_dev), static_cast<long long>(stride_bytes / 4), ctx->sh_rank,
                               ctx->F, ctx->d_ctmp.as<int>(), ctx->d_crow_len.as<int>(), ctx->d_useg.as<unsigned char>());
            MC_HIP(hipGetLastError());
            ctx->sh_pending = MC_SHARD_HIST;
            graph_build_tail(ctx);  // undo + S5 replicated, this rank's S4 tiles
        } else if (phase == MC_SHARD_HIST) {
            // src: the histogram summed over the ranks
            MC_HIP(hipMemcpyAsync(ctx->d_hist.ptr, src_dev, 8 * static_cast<size_t>(ctx->F + 1), hipMemcpyDeviceToDevice, s));
            ctx->sh_pending = 0;
            graph_build_thresholds(ctx);
        } else if (phase == MC_SHARD_FOREST) {
            MC_REQUIRE(stride_bytes % 4 == 0 && stride_bytes >= 4 * (static_cast<int64_t>(ctx->N0) + 2), MC_ERR_INVALID,
                       "bad FOREST block stride");
            {
                TimedScope ts(ctx->timer, s, "s6_pairs");
                hipLaunchKernelGGL(mc::k_sh_forest_import, dim3(grid_for(ctx->N0, 256, 1024).x, W), dim3(256), 0, s,
                                   ctx->d_Nlev.as<int>(), static_cast<const int *>(src_dev),
                                   static_cast<long long>(stride_bytes / 4), ctx->sh_rank, ctx->N0,
                                   ctx->d_parent.as<int>(), ctx->d_edges.as<unsigned long long>());
            }
            MC_HIP(hipGetLastError());
            ctx->sh_pending = 0;
            s6_iterations(ctx, 0, true);
        } else {
            throw McError{MC_ERR_INVALID, "unknown exchange phase"};
        }
    }
}

int mc_shard_export(mc_ctx *ctx, int32_t phase, void *dst_dev, int64_t *bytes)
{
    return guarded(ctx, [&] { shard_export(ctx, phase, dst_dev, bytes); });
}

int mc_shard_import(mc_ctx *ctx, int32_t phase, const void *src_dev, int64_t stride_bytes)
{
    return guarded(ctx, [&] { shard_import(ctx, phase, src_dev, stride_bytes); });
}

// ---- native collectives: RCCL, loaded on first use ------------------------------------------
namespace {
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

bool sharded(const mc_ctx *ctx) { return ctx->sh_world > 1 || ctx->comm; }
}  // namespace

// every pending exchange over the attached communicator, stream-ordered on the context stream:
// the S3 and FOREST blocks all-gathered into [world][stride] (S3's stride from a max all-reduce of
// the block sizes, one host read), the HIST block all-reduced (sum, int64)
static void shard_drain_native(mc_ctx *ctx)
{
    const Rccl &r = *rccl_lib();
    hipStream_t s = ctx->stream;
    auto comm = static_cast<ncclComm_t>(ctx->comm);
    const size_t W = static_cast<size_t>(ctx->sh_world);
    while (ctx->sh_pending) {
        const int ph = ctx->sh_pending;
        int64_t bytes = 0;
        shard_export(ctx, ph, nullptr, &bytes);
        if (ph == MC_SHARD_HIST) {
            const size_t n = static_cast<size_t>(bytes) / 8;
            ctx->d_sh_send.reserve(n * 8);
            ctx->d_sh_recv.reserve(n * 8);
            shard_export(ctx, ph, ctx->d_sh_send.ptr, &bytes);
            rccl_check(r.all_reduce(ctx->d_sh_send.ptr, ctx->d_sh_recv.ptr, n, ncclInt64, ncclSum, comm, s),
                       "ncclAllReduce (observer histogram)");
            shard_import(ctx, ph, ctx->d_sh_recv.ptr, 0);
            continue;
        }
        int64_t n_max = bytes;
        if (ph == MC_SHARD_S3) {
            ctx->d_sh_size.reserve(8);
            MC_HIP(hipMemcpy(ctx->d_sh_size.ptr, &bytes, 8, hipMemcpyHostToDevice));  // done at return
            rccl_check(r.all_reduce(ctx->d_sh_size.ptr, ctx->d_sh_size.ptr, 1, ncclInt64, ncclMax, comm, s),
                       "ncclAllReduce (S3 block size)");
            MC_HIP(hipMemcpyAsync(&n_max, ctx->d_sh_size.ptr, 8, hipMemcpyDeviceToHost, s));
            MC_HIP(hipStreamSynchronize(s));
        }
        const size_t words = static_cast<size_t>(std::max<int64_t>((n_max + 3) / 4, 1));
        ctx->d_sh_send.reserve(words * 4);
        ctx->d_sh_recv.reserve(W * words * 4);
        MC_HIP(hipMemsetAsync(ctx->d_sh_send.ptr, 0, words * 4, s));
        shard_export(ctx, ph, ctx->d_sh_send.ptr, &bytes);
        rccl_check(r.all_gather(ctx->d_sh_send.ptr, ctx->d_sh_recv.ptr, words, ncclInt32, comm, s),
                   ph == MC_SHARD_S3 ? "ncclAllGather (S3 rows)" : "ncclAllGather (union-find forests)");
        shard_import(ctx, ph, ctx->d_sh_recv.ptr, static_cast<int64_t>(4 * words));
    }
}

static void comm_detach(mc_ctx *ctx)
{
    if (ctx->comm && ctx->own_comm) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)rccl_lib()->comm_destroy(static_cast<ncclComm_t>(ctx->comm));
    }
    ctx->comm = nullptr;
    ctx->own_comm = false;
}

static void comm_attach(mc_ctx *ctx, void *comm, bool own)
{
    int rank = 0, world = 1;
    rccl_check(rccl_lib()->comm_user_rank(static_cast<ncclComm_t>(comm), &rank), "ncclCommUserRank");
    rccl_check(rccl_lib()->comm_count(static_cast<ncclComm_t>(comm), &world), "ncclCommCount");
    comm_detach(ctx);
    ctx->comm = comm;
    ctx->own_comm = own;
    ctx->sh_rank = rank;
    ctx->sh_world = world;
    ctx->sh_pending = 0;
    if (ctx->have_scene) build_s3_lists(ctx, frame_starts(ctx));
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
            ctx->sh_rank = 0;
            ctx->sh_world = 1;
            ctx->sh_pending = 0;
            if (ctx->have_scene) build_s3_lists(ctx, frame_starts(ctx));
            return;
        }
        comm_attach(ctx, nccl_comm, false);
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
        MC_HIP(hipMemcpyAsync(&cnt, ctx->d_cap_cnt.ptr, 8, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
        *n = static_cast<int64_t>(cnt);
        if (keys && cnt) {
            MC_REQUIRE(static_cast<int64_t>(cnt) <= ctx->cap_edges, MC_ERR_UNSUPPORTED,
                       "more edges than the capture capacity (raise it and run again)");
            MC_HIP(hipMemcpyAsync(keys, ctx->d_cap_buf.ptr, cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
            MC_HIP(hipStreamSynchronize(ctx->stream));
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
        if (ctx->K) MC_HIP(hipMemcpyAsync(len.data(), ctx->fin_len, ctx->K * 4, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
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
        MC_HIP(hipMemcpyAsync(sizes, ctx->d_Nlev.ptr, (ctx->n_iter + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int mc_cluster_get_level_caps(mc_ctx *ctx, int32_t *caps)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_cluster, MC_ERR_STATE, "no clustering result");
        MC_HIP(hipMemcpyAsync(caps, ctx->d_cap.ptr, (ctx->n_iter + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int mc_cluster_get_partition(mc_ctx *ctx, int32_t iteration, int32_t *labels)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_cluster, MC_ERR_STATE, "no clustering result");
        MC_REQUIRE(iteration >= 0 && iteration < ctx->n_iter, MC_ERR_INVALID, "iteration out of range");
        int nt = 0;
        MC_HIP(hipMemcpyAsync(&nt, ctx->d_Nlev.as<int>() + iteration, 4, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
        const size_t n0 = static_cast<size_t>(std::max(ctx->N0, 1));
        if (nt)
            MC_HIP(hipMemcpyAsync(labels, ctx->d_levels.as<int>() + static_cast<size_t>(iteration) * n0, nt * 4,
                                  hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int mc_cluster_get_edge_counts(mc_ctx *ctx, int64_t *edges)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->have_cluster, MC_ERR_STATE, "no clustering result");
        const size_t per = static_cast<size_t>(mc::kSpread) * mc::kSpreadStrideL;
        std::vector<unsigned long long> h(static_cast<size_t>(ctx->n_iter) * per);
        if (ctx->n_iter)
            MC_HIP(hipMemcpyAsync(h.data(), ctx->d_edges.ptr, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
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
        if (ctx->N0) MC_HIP(hipMemcpyAsync(labels, ctx->d_final_label.ptr, ctx->N0 * 4, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
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
            MC_HIP(hipMemcpyAsync(off.data(), ctx->fin_off, K * 4, hipMemcpyDeviceToHost, s));
            MC_HIP(hipMemcpyAsync(len.data(), ctx->fin_len, K * 4, hipMemcpyDeviceToHost, s));
            MC_HIP(hipMemcpyAsync(poff.data(), ctx->d_ptoff_out.ptr, (K + 1) * 4, hipMemcpyDeviceToHost, s));
            if (vf_bits && FW) MC_HIP(hipMemcpyAsync(vf_bits, ctx->fin_vf, static_cast<size_t>(K) * FW * 8, hipMemcpyDeviceToHost, s));
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
                MC_HIP(hipMemcpyAsync(pool.data(), ctx->fin_pool, end * 4, hipMemcpyDeviceToHost, s));
                MC_HIP(hipStreamSynchronize(s));
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

#include "mc_bp_host.inl"

#include "mc_pp_host.inl"

extern "C" {

// ---------------------------------------------------------------------------------------------
// instance-evaluation match counts (evaluation/evaluate.py:254-329)
// ---------------------------------------------------------------------------------------------
int mc_eval_match_counts(mc_ctx *ctx, int64_t num_points, int32_t num_pred, const uint8_t *pred_masks,
                         const int32_t *gt_instance, int32_t num_gt, const uint8_t *void_flags, int64_t *pred_verts,
                         int64_t *void_intersection, int64_t *intersection)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(num_points >= 0 && num_pred >= 0 && num_gt >= 0, MC_ERR_INVALID, "negative size");
        MC_REQUIRE((num_points == 0 || (gt_instance && void_flags && (num_pred == 0 || pred_masks))) &&
                       (num_pred == 0 || (pred_verts && void_intersection && (num_gt == 0 || intersection))),
                   MC_ERR_INVALID, "null argument");
        const int64_t P = num_points;
        const int K = num_pred, G = num_gt;
        for (int64_t p = 0; p < P; p++)
            MC_REQUIRE(gt_instance[p] >= -1 && gt_instance[p] < G, MC_ERR_INVALID, "gt instance index out of range");
        hipStream_t s = ctx->stream;
        DevBuf dpred, dg, dv, dverts, dvi, dint;
        dpred.reserve(static_cast<size_t>(P) * K + 8);
        dg.reserve(P * 4 + 8);
        dv.reserve(P + 8);
        dverts.reserve(K * 8 + 8);
        dvi.reserve(K * 8 + 8);
        dint.reserve(static_cast<size_t>(K) * G * 8 + 8);
        if (P && K) MC_HIP(hipMemcpyAsync(dpred.ptr, pred_masks, static_cast<size_t>(P) * K, hipMemcpyHostToDevice, s));
        if (P) {
            MC_HIP(hipMemcpyAsync(dg.ptr, gt_instance, P * 4, hipMemcpyHostToDevice, s));
            MC_HIP(hipMemcpyAsync(dv.ptr, void_flags, P, hipMemcpyHostToDevice, s));
        }
        MC_HIP(hipMemsetAsync(dverts.ptr, 0, K * 8 + 8, s));
        MC_HIP(hipMemsetAsync(dvi.ptr, 0, K * 8 + 8, s));
        MC_HIP(hipMemsetAsync(dint.ptr, 0, static_cast<size_t>(K) * G * 8 + 8, s));
        {
            mc::TimedScope ts(ctx->timer, s, "eval_counts");
            if (P && K)
                hipLaunchKernelGGL(mc::k_eval_counts, grid_for(P, 256, 8192), dim3(256), 0, s, P, K, G, dpred.as<unsigned char>(),
                                   dg.as<int>(), dv.as<unsigned char>(), dverts.as<unsigned long long>(),
                                   dvi.as<unsigned long long>(), dint.as<unsigned long long>());
            MC_HIP(hipGetLastError());
        }
        if (K) {
            MC_HIP(hipMemcpyAsync(pred_verts, dverts.ptr, K * 8, hipMemcpyDeviceToHost, s));
            MC_HIP(hipMemcpyAsync(void_intersection, dvi.ptr, K * 8, hipMemcpyDeviceToHost, s));
            if (G) MC_HIP(hipMemcpyAsync(intersection, dint.ptr, static_cast<size_t>(K) * G * 8, hipMemcpyDeviceToHost, s));
        }
        MC_HIP(hipStreamSynchronize(s));
        ctx->timer.collect();
    });
}


// ---------------------------------------------------------------------------------------------
// frame decode (dataset/scannet.py:49-54, :68-73)
// ---------------------------------------------------------------------------------------------
int mc_frames_decode(mc_ctx *ctx, int32_t num_frames, int32_t height, int32_t width, const uint16_t *depth,
                     double depth_scale, int32_t seg_height, int32_t seg_width, const uint8_t *seg, int inputs_on_device,
                     float *depth_out, uint8_t *seg_out)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(num_frames >= 0 && height >= 0 && width >= 0 && seg_height >= 0 && seg_width >= 0, MC_ERR_INVALID,
                   "negative size");
        MC_REQUIRE((!depth || (depth_out && depth_scale != 0.0)) && (!seg || (seg_out && seg_height > 0 && seg_width > 0)),
                   MC_ERR_INVALID, "missing output or bad scale");
        const int64_t total = static_cast<int64_t>(num_frames) * height * width;
        const int64_t stotal = static_cast<int64_t>(num_frames) * seg_height * seg_width;
        // cv2.resize(..., INTER_NEAREST) tables (OpenCV resizeNN): src = min(floor(dst * (1 / (dsize / ssize))), ssize - 1)
        std::vector<int> yo(std::max(height, 1)), xo(std::max(width, 1));
        const double ify = 1.0 / (static_cast<double>(height) / seg_height), ifx = 1.0 / (static_cast<double>(width) / seg_width);
        for (int y = 0; y < height; y++) yo[y] = std::min(static_cast<int>(std::floor(y * ify)), seg_height - 1);
        for (int x = 0; x < width; x++) xo[x] = std::min(static_cast<int>(std::floor(x * ifx)), seg_width - 1);
        hipStream_t s = ctx->stream;
        DevBuf dd, ds, dyo, dxo;
        const unsigned short *din = reinterpret_cast<const unsigned short *>(depth);
        const unsigned char *sin = seg;
        if (!inputs_on_device) {
            if (depth) {
                dd.reserve(total * 2 + 8);
                if (total) MC_HIP(hipMemcpyAsync(dd.ptr, depth, total * 2, hipMemcpyHostToDevice, s));
                din = dd.as<unsigned short>();
            }
            if (seg) {
                ds.reserve(stotal + 8);
                if (stotal) MC_HIP(hipMemcpyAsync(ds.ptr, seg, stotal, hipMemcpyHostToDevice, s));
                sin = ds.as<unsigned char>();
            }
        }
        dyo.reserve(yo.size() * 4);
        dxo.reserve(xo.size() * 4);
        MC_HIP(hipMemcpyAsync(dyo.ptr, yo.data(), yo.size() * 4, hipMemcpyHostToDevice, s));
        MC_HIP(hipMemcpyAsync(dxo.ptr, xo.data(), xo.size() * 4, hipMemcpyHostToDevice, s));
        {
            mc::TimedScope ts(ctx->timer, s, "frames_decode");
            if (total && (depth || seg))
                hipLaunchKernelGGL(mc::k_frames_decode, grid_for(total, 256, 16384), dim3(256), 0, s, total, height, width,
                                   seg_height, seg_width, depth ? din : nullptr, depth_scale, seg ? sin : nullptr,
                                   dyo.as<int>(), dxo.as<int>(), depth_out, seg_out);
            MC_HIP(hipGetLastError());
        }
        MC_HIP(hipStreamSynchronize(s));
        ctx->timer.collect();
    });
}

// ---------------------------------------------------------------------------------------------
// host: packed bit rows -> bool bytes (the reference's dense point_frame_matrix, construction.py:40)
// ---------------------------------------------------------------------------------------------
int mc_bits_unpack(const uint64_t *words, int64_t rows, int32_t words_per_row, int32_t ncols, uint8_t *out)
{
    if (rows < 0 || words_per_row < 0 || ncols < 0 || static_cast<int64_t>(ncols) > 64ll * words_per_row)
        return MC_ERR_INVALID;
    if (!rows || !ncols) return MC_OK;
    if (!words || !out) return MC_ERR_INVALID;
    static const auto lut = [] {  // byte value -> its 8 bits as 8 bytes (little-endian)
        std::vector<uint64_t> t(256);
        for (int v = 0; v < 256; v++) {
            uint64_t x = 0;
            for (int b = 0; b < 8; b++) x |= static_cast<uint64_t>((v >> b) & 1) << (8 * b);
            t[v] = x;
        }
        return t;
    }();
    auto work = [&](int64_t r0, int64_t r1) {
        const int full = ncols / 8;  // whole output bytes groups of 8 columns
        for (int64_t r = r0; r < r1; r++) {
            const uint8_t *wb = reinterpret_cast<const uint8_t *>(words + r * words_per_row);
            uint8_t *o = out + r * ncols;
            for (int j = 0; j < full; j++) {
                const uint64_t x = lut[wb[j]];
                memcpy(o + 8 * j, &x, 8);
            }
            for (int c = 8 * full; c < ncols; c++) o[c] = static_cast<uint8_t>((wb[c >> 3] >> (c & 7)) & 1u);
        }
    };
    const int64_t bytes = rows * ncols;
    int nt = static_cast<int>(std::min<int64_t>(std::min(8u, std::max(1u, std::thread::hardware_concurrency())),
                                                std::max<int64_t>(1, bytes >> 22)));
    nt = stage_threads_knob(nt);
    if (nt <= 1) {
        work(0, rows);
        return MC_OK;
    }
    std::vector<std::thread> th;
    const int64_t step = (rows + nt - 1) / nt;
    for (int t = 1; t < nt; t++) th.emplace_back(work, std::min(rows, t * step), std::min(rows, (t + 1) * step));
    work(0, std::min(rows, step));
    for (auto &x : th) x.join();
    return MC_OK;
}

// ---------------------------------------------------------------------------------------------
// open-vocabulary label query
// ---------------------------------------------------------------------------------------------
int mc_openvoc_query(mc_ctx *ctx, int32_t num_objects, const int64_t *obj_off, const int32_t *obj_rows,
                     int32_t num_rows, int32_t dim, const float *features, int32_t num_labels,
                     const float *label_features, float temperature, int32_t *out_label)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(num_objects >= 0 && num_rows >= 0 && dim > 0 && dim <= 12288 && num_labels > 0, MC_ERR_INVALID,
                   "bad sizes");
        MC_REQUIRE(obj_off && out_label && label_features && (num_rows == 0 || features), MC_ERR_INVALID, "null array");
        MC_REQUIRE(obj_off[0] == 0, MC_ERR_INVALID, "obj_off[0] != 0");
        const int64_t nr = obj_off[num_objects];
        MC_REQUIRE(nr == 0 || obj_rows, MC_ERR_INVALID, "null array");
        for (int k = 0; k < num_objects; k++) MC_REQUIRE(obj_off[k + 1] >= obj_off[k], MC_ERR_INVALID, "obj_off not ascending");
        for (int64_t i = 0; i < nr; i++)
            MC_REQUIRE(obj_rows[i] >= 0 && obj_rows[i] < num_rows, MC_ERR_INVALID, "feature row out of range");
        if (!num_objects) return;
        hipStream_t s = ctx->stream;
        DevBuf doff, drows, dfeat, dlab, dsim, dout;
        doff.reserve((num_objects + 1) * 8);
        drows.reserve((nr + 1) * 4);
        dfeat.reserve(static_cast<size_t>(num_rows) * dim * 4 + 4);
        dlab.reserve(static_cast<size_t>(num_labels) * dim * 4);
        dsim.reserve(static_cast<size_t>(num_objects) * num_labels * 4);
        dout.reserve(static_cast<size_t>(num_objects) * 4);
        MC_HIP(hipMemcpyAsync(doff.ptr, obj_off, (num_objects + 1) * 8, hipMemcpyHostToDevice, s));
        if (nr) MC_HIP(hipMemcpyAsync(drows.ptr, obj_rows, nr * 4, hipMemcpyHostToDevice, s));
        if (num_rows) MC_HIP(hipMemcpyAsync(dfeat.ptr, features, static_cast<size_t>(num_rows) * dim * 4, hipMemcpyHostToDevice, s));
        MC_HIP(hipMemcpyAsync(dlab.ptr, label_features, static_cast<size_t>(num_labels) * dim * 4, hipMemcpyHostToDevice, s));
        {
            TimedScope ts(ctx->timer, s, "ov_query");
            hipLaunchKernelGGL(mc::k_ov_query, dim3(num_objects), dim3(256), dim * sizeof(float), s, num_objects,
                               doff.as<long long>(), drows.as<int>(), dim, dfeat.as<float>(), num_labels,
                               dlab.as<float>(), temperature, dsim.as<float>(), dout.as<int>());
        }
        MC_HIP(hipGetLastError());
        MC_HIP(hipMemcpyAsync(out_label, dout.ptr, static_cast<size_t>(num_objects) * 4, hipMemcpyDeviceToHost, s));
        MC_HIP(hipStreamSynchronize(s));
    });
}

}  // extern "C"

#include "mc_ap_host.inl"
