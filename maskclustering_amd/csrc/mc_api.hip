// mc_api.hip — C-ABI of libmcgraph, the single translation unit: the includes, the error guard and the
// helpers every driver uses (fail, guarded, grid_for, sync_stats, fetch), the context's lifecycle and timing
// entries (mc_ctx_*), the host-driver includes, and the four small stateless entries.  The context and its
// state structs are mc_ctx.hpp, the kernels live in mc_*kernels.inl (mc_kernels.inl and mc_bp_kernels.inl
// are umbrellas of one file per stage), the host drivers in mc_*_host.inl, the decisions they take between
// kernels in mc_*_plan.hpp.
#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the library loads RCCL at mc_ctx_attach_comm / mc_ctx_comm_init (dlopen)

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "mc_internal.hpp"
#include "mc_bp_nbpack.hpp"
#include "mc_bp_plan.hpp"
#include "mc_graph_plan.hpp"
#include "mc_pp_plan.hpp"
#include "mc_ap_plan.hpp"
#include "mc_crop_plan.hpp"
#include "mc_proj_plan.hpp"
#include "mc_cloud_plan.hpp"
#include "mc_paint_plan.hpp"
#include "mc_kernels.inl"
#include "mc_bp_kernels.inl"
#include "mc_pp_kernels.inl"
#include "mc_eval_kernels.inl"
#include "mc_ap_kernels.inl"
#include "mc_io_kernels.inl"
#include "mc_shard_kernels.inl"
#include "mc_ov_kernels.inl"
#include "mc_crop_kernels.inl"
#include "mc_proj_kernels.inl"
#include "mc_cloud_kernels.inl"
#include "mc_paint_kernels.inl"
#include "mc_setorder.inl"

using mc::DevBuf;
using mc::EvTables;
using mc::McError;
using mc::TimedScope;
using mc::ceil_div;

#include "mc_ctx.hpp"

namespace {

// MC_STAGE_THREADS: host threads of the staging copies (mc_backproject_frames, mc_bits_unpack)
int stage_threads_knob(int dflt)
{
    if (const char *e = getenv("MC_STAGE_THREADS")) return std::max(1, std::min(64, atoi(e)));
    return dflt;
}

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

// a device array to the host, waited for (nothing to copy: the wait alone)
void fetch(mc_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (bytes) MC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MC_HIP(hipStreamSynchronize(ctx->stream));
}

// mc_shard_host.inl
bool sharded(const mc_ctx *ctx);
void shard_drain_native(mc_ctx *ctx);
void comm_detach(mc_ctx *ctx);

}  // namespace

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
        MC_HIP(hipDeviceGetAttribute(&ctx->max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
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
    if (ctx->shard.comm) {
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

}  // extern "C"

// the host drivers (template kernels are emitted in the order of their first use: keep this order)
#include "mc_graph_host.inl"
#include "mc_cluster_host.inl"
#include "mc_shard_host.inl"
#include "mc_bp_host.inl"
#include "mc_pp_host.inl"
#include "mc_ap_host.inl"
#include "mc_crop_host.inl"
#include "mc_proj_host.inl"
#include "mc_cloud_host.inl"
#include "mc_paint_host.inl"

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
