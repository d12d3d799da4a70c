// mc_bp_host.inl — S1 back-projection: the host side (included by mc_api.hip, same translation unit).
// bp_run drives one call: plan the batches (mc_bp_plan.hpp), then per batch launch the pixel, voxel,
// denoise and query groups, check the status block, and emit and pack the batch's masks; the public
// entries at the end validate, describe where the frames are (BpFrames) and call it.
extern "C" {

__global__ void k_fill_u32(unsigned *p, size_t n, unsigned v)
{
    for (size_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * 256) p[i] = v;
}

}  // extern "C"

namespace {

using mc::kBpBytesPerFramePixel;
using mc::kBpBytesPerMaskPixel;

void fill_u32(hipStream_t s, void *p, size_t n, unsigned v)
{
    if (n) hipLaunchKernelGGL(k_fill_u32, grid_for(static_cast<int64_t>(n)), dim3(256), 0, s, static_cast<unsigned *>(p), n, v);
}

// grow a device buffer, keeping its first `used` bytes
void grow_keep(DevBuf &b, size_t bytes, size_t used, hipStream_t s)
{
    if (bytes <= b.bytes) return;
    DevBuf nb;
    nb.reserve(bytes + bytes / 2);
    if (used) MC_HIP(hipMemcpyAsync(nb.ptr, b.ptr, used, hipMemcpyDeviceToDevice, s));
    MC_HIP(hipStreamSynchronize(s));
    b.swap(nb);  // the old buffer is freed with nb
}

enum BpStat : int {
    BS_ERRF = 0, BS_VOXERR, BS_OVF, BS_TOP, BS_NS, BS_NPX, BS_M, BS_NNZ,
    BS_CLS,             // denoise size-class counts (kBpClasses LDS classes + the global-memory kernel)
    BS_TK = BS_CLS + mc::kBpClasses + 1,  // ticket counters of the LDS classes
    BS_VXFB = BS_TK + mc::kBpClasses,     // slots the first voxel tier hands to the second
    BS_VXFB2,                             // slots the second voxel tier hands to k_bp_voxel
    BS_DQ,                                // points queued for the k-NN ring search
    BS_DNERR,                             // denoise internal-error bits (queue entry / region out of range)
    BS_PXOVF,                             // the batch's mask pixels exceed the capacity: grown, batch redone
    BS_QFB,                               // slots the staged ball query hands to k_bp_query
    BS_COUNT
};

size_t slots_cap(int fb) { return static_cast<size_t>(fb) * 256 + 1; }  // (frame, id) slots of a batch

// Workgroups per resident slot of a denoise class (the classes take slots from tickets): the extra
// ones start on CUs that other classes free, so no class keeps only its initial share of the chip.
#ifndef MC_BP_OVERSUB
#define MC_BP_OVERSUB 2
#endif
constexpr int kBpOversub = MC_BP_OVERSUB;  // class grids: resident workgroups x this (slots come from tickets)

// The capacities of the denoise's LDS size classes, ascending (class index = position): mc::kBpClassN
// (mc_bp_denoise_lds.inl), the list k_bp_classify's thresholds read too.  mc::BpLdsClass<N> gives each
// class's shape.
using mc::kBpClassN;
constexpr int bp_class_index(int N)
{
    for (int c = 0; c < mc::kBpClasses; c++)
        if (kBpClassN[c] == N) return c;
    return -1;
}

// Per-workgroup arrays before class cls's region (cls = kBpClasses: the whole array), one fold over the
// list: u16 entries of eps-neighbour lists (kBpNbCap per point), or ints of lean scratch
template <size_t... I>
constexpr size_t bp_class_fold(int cls, bool lean, std::index_sequence<I...>)
{
    return ((static_cast<int>(I) < cls ? (lean ? mc::kBpLeanInts<kBpClassN[I]> : static_cast<size_t>(kBpClassN[I]) * mc::kBpNbCap) *
                                             mc::BpLdsClass<kBpClassN[I]>::kWgPerCu : 0) + ...);
}
inline size_t bp_class_offset(const mc_ctx *ctx, int cls, bool lean)
{
    return bp_class_fold(cls, lean, std::make_index_sequence<mc::kBpClasses>{}) * ctx->num_cu * kBpOversub;
}
inline size_t nbl_offset(const mc_ctx *ctx, int cls) { return bp_class_offset(ctx, cls, false); }
inline size_t lean_offset(const mc_ctx *ctx, int cls) { return bp_class_offset(ctx, cls, true); }

// workgroups per CU of k_bp_query: it waits on dependent cell-range and point loads, so as many waves
// as the registers allow (the 20-entry best list of ball_k <= 20: 76 VGPRs, six workgroups per CU, C3
// query 8.4 -> 6.5 ms per scene; 32 entries: 89 VGPRs, five).  One point bitmap per workgroup.
constexpr int kBpQueryWgPerCu20 = 6, kBpQueryWgPerCu32 = 5;
constexpr int kBpQueryWgPerCuMax = std::max(kBpQueryWgPerCu20, kBpQueryWgPerCu32);
// workgroups per CU of k_bp_query_lds: its 30.8 KB of LDS (the crop, the cell table, the staging list /
// accepted ids and flags) fit five times into a CU's 160 KB
constexpr int kBpQueryLdsWgPerCu = 5;

// Test and tuning knobs of S1, read at the start of every call (tests change them between calls on
// one context)
struct BpKnobs {
    int min_cls = 0;    // MC_BP_MIN_CLASS: smallest denoise size class (0 = by size; kBpClasses = the global-memory kernel)
    int vx_global = 0;  // MC_VX_GLOBAL: 1 hands every slot to the global-hash voxel kernel, 2 to the second LDS tier
    bool fixed_batch = false;  // MC_BP_BATCH_PIXELS: batch_pixels frame pixels per batch, whatever the byte budget
    size_t batch_pixels = 0;
    int upload_batches = 1;    // MC_BP_UPLOAD_BATCHES: frames staged from the host take at least this many batches
    // MC_KNN_RADII="a,b,c": k-NN pre-selection radii (fractions of eps, ascending, < 1): any choice gives
    // the same results (the smallest radius holding >= k kept points is used)
    double knn_fr[3] = {0.6, 0.75, 0.9};
    int nbcap = mc::kBpNbCap;  // MC_BP_NBCAP: eps lists read only up to this many entries (the rest take the cell walks)
    int tail_wg = 8;           // MC_BP_TAILWG: workgroups per CU of k_bp_denoise_tail
    int stage_threads = 1;     // MC_STAGE_THREADS: host threads filling the pinned staging chunks
    // the staged ball query (k_bp_query_lds): MC_BP_QUERY_STAGED=0 hands every slot to k_bp_query;
    // MC_BP_QUERY_CELLS / MC_BP_QUERY_CAND: a slot with more box cells / cropped scene points goes to
    // k_bp_query (at most the compiled LDS sizes); MC_BP_QUERY_GRID: its workgroups in all (0 = by CU
    // count; 1 makes one workgroup take every slot in turn)
    bool q_staged = true;
    int q_cells = mc::kBpQcCells, q_cand = mc::kBpQcCand, q_grid = 0;
    bool q_report = false;     // MC_BP_QUERY_REPORT=1: per batch, the slots and how many took k_bp_query (stderr)
};

BpKnobs bp_read_knobs(mc_ctx *ctx)
{
    BpKnobs k;
    if (const char *e = getenv("MC_BP_MIN_CLASS")) k.min_cls = std::min(mc::kBpClasses, std::max(0, atoi(e)));
    if (const char *e = getenv("MC_VX_GLOBAL")) k.vx_global = atoi(e);
    // MC_BP_MASK_FRAC sets the expected mask-pixel share (a small one forces the grow-and-redo path)
    if (const char *e = getenv("MC_BP_MASK_FRAC")) ctx->bp.mfrac = atof(e);
    if (const char *e = getenv("MC_BP_BATCH_PIXELS")) {
        k.fixed_batch = true;
        k.batch_pixels = std::max<size_t>(1, strtoull(e, nullptr, 10));
    }
    if (const char *e = getenv("MC_BP_UPLOAD_BATCHES")) k.upload_batches = std::max(1, atoi(e));
    if (const char *e = getenv("MC_KNN_RADII")) {
        double a[3];
        if (sscanf(e, "%lf,%lf,%lf", &a[0], &a[1], &a[2]) == 3 && 0 < a[0] && a[0] < a[1] && a[1] < a[2] && a[2] < 1)
            for (int i = 0; i < 3; i++) k.knn_fr[i] = a[i];
    }
    if (const char *e = getenv("MC_BP_NBCAP")) k.nbcap = std::min(mc::kBpNbCap, std::max(1, atoi(e)));
    if (const char *e = getenv("MC_BP_TAILWG")) k.tail_wg = std::max(1, atoi(e));
    if (const char *e = getenv("MC_BP_QUERY_STAGED")) k.q_staged = atoi(e) != 0;
    if (const char *e = getenv("MC_BP_QUERY_CELLS")) k.q_cells = std::min(mc::kBpQcCells, std::max(1, atoi(e)));
    if (const char *e = getenv("MC_BP_QUERY_CAND")) k.q_cand = std::min(mc::kBpQcCand, std::max(0, atoi(e)));
    if (const char *e = getenv("MC_BP_QUERY_GRID")) k.q_grid = std::max(1, atoi(e));
    if (const char *e = getenv("MC_BP_QUERY_REPORT")) k.q_report = atoi(e) != 0;
    k.stage_threads = stage_threads_knob(static_cast<int>(std::min(8u, std::max(1u, std::thread::hardware_concurrency()))));
    return k;
}

// (re)allocate the per-batch arrays for fb frames of H x W and mask_px mask pixels
void bp_reserve(mc_ctx *ctx, int fb, int H, int W, int nbands, size_t mask_px, hipStream_t s)
{
    BpState &bp = ctx->bp;
    const size_t px = mask_px + 1;
    const size_t slots = slots_cap(fb);
    bp.band.reserve(static_cast<size_t>(fb) * nbands * mc::kBpWaves * 256 * 4);
    bp.vid.reserve(static_cast<size_t>(fb) * H * W + 16);
    bp.fpx_cap = std::max(bp.fpx_cap, static_cast<size_t>(fb) * H * W);
    bp.present.reserve(static_cast<size_t>(fb) * 8 * 4);
    bp.fflags.reserve(static_cast<size_t>(fb) * 4);
    bp.stat.reserve(BS_COUNT * 4);
    for (DevBuf *b : {&bp.cand, &bp.npix, &bp.slot_of, &bp.slot_frame, &bp.slot_id, &bp.slot_np, &bp.slot_pix, &bp.slot_nv,
                      &bp.slot_m, &bp.slot_ns, &bp.slot_nn, &bp.slot_toff, &bp.slot_cov, &bp.kflag, &bp.ksize, &bp.vox_order,
                      &bp.q_fb})
        b->reserve(slots * 4);
    for (DevBuf *b : {&bp.csidx, &bp.poff, &bp.midx, &bp.moff}) b->reserve((slots + 1) * 4);
    bp.slot_box.reserve(slots * 6 * 4);
    bp.cls_list.reserve((mc::kBpClasses + 1) * slots * 4);
    bp.vx_fb.reserve(2 * slots * 4);  // the two tiers' overflow lists
    bp.scanm.reserve(4 * (slots / mc::kScanTile + 3) * 4);
    bp.slot_grid.reserve(8 * slots * 8);
    // per-workgroup eps-neighbour lists, one region per size class (the classes run concurrently)
    bp.nbl.reserve(nbl_offset(ctx, mc::kBpClasses) * 2);
    bp.lean.reserve(lean_offset(ctx, mc::kBpClasses) * 4);
    if (bp.px_cap < px) {
        for (DevBuf *b : {&bp.pix_list, &bp.vx_pvid, &bp.vx_list, &bp.vox_entry, &bp.pbkt, &bp.blist, &bp.ncnt, &bp.par,
                          &bp.droot, &bp.rnk, &bp.lab, &bp.ssidx})
            b->reserve(px * 4);
        for (DevBuf *b : {&bp.hvid, &bp.hfirst, &bp.bcnt, &bp.pcell, &bp.avg}) b->reserve(2 * px * 4);
        bp.hkey.reserve(2 * px * 8);
        fill_u32(s, bp.hkey.ptr, 4 * px, 0xFFFFFFFFu);    // empty key, kept empty by k_bp_voxel
        fill_u32(s, bp.hvid.ptr, 2 * px, 0xFFFFFFFFu);    // -1
        fill_u32(s, bp.hfirst.ptr, 2 * px, 0x7FFFFFFFu);  // INT_MAX
        fill_u32(s, bp.bcnt.ptr, 2 * px, 0u);             // kept zero by k_bp_denoise
        bp.acc.reserve(px * 4 * 8);
        bp.vpts.reserve(px * 3 * 8);
        bp.qpts.reserve(px * 3 * 4);
        bp.bstart.reserve((2 * px + slots + 1) * 4);
        bp.ccnt.reserve((px + slots + 1) * 4);
        bp.px_cap = px;
    }
}

void bp_build_grid(mc_ctx *ctx, float radius, hipStream_t s)
{
    BpState &bp = ctx->bp;
    const int P = static_cast<int>(bp.P);
    const float inv = 1.0f / (2.0f * radius);
    const unsigned nb = static_cast<unsigned>(std::max(2 * P, 16));
    bp.gnb = nb;
    const bool fresh = bp.gcnt.bytes < (nb + 1) * 4ull;
    bp.gcnt.reserve((nb + 1) * 4ull);
    if (fresh) MC_HIP(hipMemsetAsync(bp.gcnt.ptr, 0, bp.gcnt.bytes, s));  // kept zero by k_grid_scatter
    bp.gstart.reserve((nb + 2) * 4ull);
    bp.gbkt.reserve((P + 1) * 4ull);
    bp.gcellk.reserve((P + 1) * 8ull);
    bp.gpts.reserve((P + 1) * 16ull);
    bp.gidx.reserve((P + 1) * 4ull);
    bp.gcell.reserve((P + 1) * 8ull);
    bp.gscan_tmp.reserve((2 * (nb / mc::kScanTile + 4) + 16) * 4ull);
    if (P) {
        hipLaunchKernelGGL(mc::k_grid_count, grid_for(P), dim3(256), 0, s, bp.scene.as<float>(), P, inv, nb,
                           bp.gcnt.as<int>(), bp.gbkt.as<unsigned>(), bp.gcellk.as<unsigned long long>());
    }
    mc::scan_large(s, bp.gcnt.as<int>(), bp.gstart.as<int>(), static_cast<int>(nb), bp.gscan_tmp.as<int>());
    if (P)
        hipLaunchKernelGGL(mc::k_grid_scatter, grid_for(P), dim3(256), 0, s, bp.scene.as<float>(), P,
                           bp.gbkt.as<unsigned>(), bp.gcellk.as<unsigned long long>(), bp.gstart.as<int>(),
                           bp.gcnt.as<int>(), bp.gpts.as<float4>(), bp.gidx.as<int>(),
                           bp.gcell.as<unsigned long long>());
    bp.grid_radius = radius;
}

// MC_BP_DEBUG_SYNC=1: synchronise and report after every S1 group (diagnostics of a stalled batch)
void bp_debug_sync(hipStream_t s, const char *what)
{
    static const bool on = getenv("MC_BP_DEBUG_SYNC") != nullptr;
    if (!on) return;
    fprintf(stderr, "[mc bp] %s issued\n", what);
    MC_HIP(hipStreamSynchronize(s));
    MC_HIP(hipDeviceSynchronize());
    fprintf(stderr, "[mc bp] %s done\n", what);
}

// Where a call's frames are: device arrays, contiguous host arrays (copied up at once), or per-frame host arrays, staged batch
// by batch on the copy stream while the previous batch computes: frames [0, staged) are on the
// device (or queued on bp.copy before bp.ev_up).
struct BpFrames {
    enum Kind { kDevice, kHost, kHostFrames } kind = kDevice;
    const float *depth = nullptr;  // [F, H, W] of kDevice / kHost; the device arrays once bp_bind_frames ran
    const uint8_t *seg = nullptr;
    const void *const *depth_frames = nullptr;  // kHostFrames: frames[f] = host pointer of frame f
    const void *const *seg_frames = nullptr;
    const double *intr = nullptr, *pose = nullptr;
    double raw_scale = 0.0;  // > 0: depth frames are the PNGs' uint16 values, decoded on the copy stream
    int staged = 0;
    bool given(int F) const
    {
        if (!intr || !pose) return false;
        if (kind != kHostFrames) return depth && seg;
        for (int f = 0; depth_frames && seg_frames && f < F; f++)
            if (!depth_frames[f] || !seg_frames[f]) return false;
        return depth_frames && seg_frames;
    }
};

// Per-frame host arrays -> one device array [F, frame_bytes]: frames [f_lo, f_hi) -> dst + f *
// frame_bytes, through the pinned ping-pong chunks: host threads fill one chunk while the DMA of the
// other runs on stream s (pageable hipMemcpy would stage through the runtime's own buffers on one
// thread, and np.stack would add a full host copy)
void stage_frames(mc_ctx *ctx, const void *const *frames, size_t frame_bytes, int f_lo, int f_hi, char *dst,
                  hipStream_t s, int nthreads)
{
    BpState &bp = ctx->bp;
    if (f_hi <= f_lo || !frame_bytes) return;
    const size_t want = std::max<size_t>(frame_bytes, static_cast<size_t>(32) << 20);
    if (bp.stage_bytes < want) {
        for (int b = 0; b < 2; b++) {
            if (bp.stage_used[b]) MC_HIP(hipEventSynchronize(bp.ev_stage[b]));
            if (bp.h_stage[b]) MC_HIP(hipHostFree(bp.h_stage[b]));
            bp.h_stage[b] = nullptr;
            bp.stage_used[b] = false;
        }
        bp.stage_bytes = 0;
        for (int b = 0; b < 2; b++) {
            MC_HIP(hipHostMalloc(reinterpret_cast<void **>(&bp.h_stage[b]), want, hipHostMallocDefault));
            if (!bp.ev_stage[b]) MC_HIP(hipEventCreateWithFlags(&bp.ev_stage[b], hipEventDisableTiming));
        }
        bp.stage_bytes = want;
    }
    const int per = static_cast<int>(std::max<size_t>(1, bp.stage_bytes / frame_bytes));
    int b = 0;
    for (int f0 = f_lo; f0 < f_hi; f0 += per, b ^= 1) {
        const int n = std::min(per, f_hi - f0);
        if (bp.stage_used[b]) MC_HIP(hipEventSynchronize(bp.ev_stage[b]));  // its last DMA is done
        char *buf = bp.h_stage[b];
        const size_t total = static_cast<size_t>(n) * frame_bytes;
        auto copy_range = [&](size_t lo, size_t hi) {
            while (lo < hi) {
                const size_t f = lo / frame_bytes, o = lo % frame_bytes;
                const size_t len = std::min(hi - lo, frame_bytes - o);
                memcpy(buf + lo, static_cast<const char *>(frames[f0 + f]) + o, len);
                lo += len;
            }
        };
        const int nt = static_cast<int>(std::min<size_t>(nthreads, std::max<size_t>(1, total >> 22)));  // >= 4 MB each
        if (nt <= 1) {
            copy_range(0, total);
        } else {
            std::vector<std::thread> th;
            const size_t step = (total + nt - 1) / nt;
            for (int t = 1; t < nt; t++) th.emplace_back(copy_range, std::min(total, t * step), std::min(total, (t + 1) * step));
            copy_range(0, std::min(total, step));
            for (auto &x : th) x.join();
        }
        MC_HIP(hipMemcpyAsync(dst + static_cast<size_t>(f0) * frame_bytes, buf, total, hipMemcpyHostToDevice, s));
        MC_HIP(hipEventRecord(bp.ev_stage[b], s));
        bp.stage_used[b] = true;
    }
}

// the call's frames as device arrays: host arrays go into the context's in_* buffers (per-frame ones
// only get their room here; bp_stage_to fills it)
void bp_bind_frames(mc_ctx *ctx, BpFrames &src, int F, size_t HW, hipStream_t s)
{
    BpState &bp = ctx->bp;
    if (src.kind == BpFrames::kDevice || !F) return;
    bp.in_depth.reserve(F * HW * 4);
    bp.in_seg.reserve(F * HW);
    bp.in_intr.reserve(F * 4 * 8ull);
    bp.in_pose.reserve(F * 16 * 8ull);
    if (src.kind == BpFrames::kHost) {
        MC_HIP(hipMemcpyAsync(bp.in_depth.ptr, src.depth, F * HW * 4, hipMemcpyHostToDevice, s));
        MC_HIP(hipMemcpyAsync(bp.in_seg.ptr, src.seg, F * HW, hipMemcpyHostToDevice, s));
    } else {
        if (src.raw_scale > 0.0) bp.in_raw.reserve(F * HW * 2);
        if (!bp.copy) {
            MC_HIP(hipStreamCreateWithFlags(&bp.copy, hipStreamNonBlocking));
            MC_HIP(hipEventCreateWithFlags(&bp.ev_up, hipEventDisableTiming));
        }
    }
    MC_HIP(hipMemcpyAsync(bp.in_intr.ptr, src.intr, F * 4 * 8ull, hipMemcpyHostToDevice, s));
    MC_HIP(hipMemcpyAsync(bp.in_pose.ptr, src.pose, F * 16 * 8ull, hipMemcpyHostToDevice, s));
    src.depth = bp.in_depth.as<float>();
    src.seg = bp.in_seg.as<uint8_t>();
    src.intr = bp.in_intr.as<double>();
    src.pose = bp.in_pose.as<double>();
}

// stage the host frames [src.staged, f_hi) on the copy stream
void bp_stage_to(mc_ctx *ctx, BpFrames &src, int f_hi, int H, int W, int nthreads)
{
    BpState &bp = ctx->bp;
    if (src.kind != BpFrames::kHostFrames || f_hi <= src.staged) return;
    const size_t HW = static_cast<size_t>(H) * W;
    if (src.raw_scale > 0.0) {  // 2-byte frames, then float32(u16 / scale) on the copy stream
        stage_frames(ctx, src.depth_frames, HW * 2, src.staged, f_hi, static_cast<char *>(bp.in_raw.ptr), bp.copy, nthreads);
        const int64_t total = static_cast<int64_t>(f_hi - src.staged) * static_cast<int64_t>(HW);
        hipLaunchKernelGGL(mc::k_frames_decode, grid_for(total, 256, 16384), dim3(256), 0, bp.copy, total, H, W, 1, 1,
                           bp.in_raw.as<unsigned short>() + static_cast<size_t>(src.staged) * HW, src.raw_scale,
                           static_cast<const unsigned char *>(nullptr), static_cast<const int *>(nullptr),
                           static_cast<const int *>(nullptr),
                           bp.in_depth.as<float>() + static_cast<size_t>(src.staged) * HW,
                           static_cast<unsigned char *>(nullptr));
        MC_HIP(hipGetLastError());
    } else {
        stage_frames(ctx, src.depth_frames, HW * 4, src.staged, f_hi, static_cast<char *>(bp.in_depth.ptr), bp.copy, nthreads);
    }
    stage_frames(ctx, src.seg_frames, HW, src.staged, f_hi, static_cast<char *>(bp.in_seg.ptr), bp.copy, nthreads);
    MC_HIP(hipEventRecord(bp.ev_up, bp.copy));
    src.staged = f_hi;
}

// the kernels' parameter block.  vec4: the pixel kernels' uchar4 / float4 loads need aligned frames (a
// caller's tensor view may start at any element); every batch starts HW pixels further on, a multiple
// of 4 when W is
mc::BpDev bp_make_dev(const mc_bp_params &prm, const BpKnobs &kn, int H, int W, int nbands, const float *dep,
                      const uint8_t *sg)
{
    const float rf = static_cast<float>(prm.ball_radius);
    mc::BpDev dv;
    dv.trunc = prm.depth_trunc;
    dv.vs = prm.voxel_size;
    dv.rvs = 1.0 / prm.voxel_size;  // (IEEE division on the host: RN(1 / vs), div_rn's reciprocal)
    dv.eps2 = prm.dbscan_eps * prm.dbscan_eps;
    for (int i = 0; i < 3; i++) dv.knn_r2[i] = (kn.knn_fr[i] * prm.dbscan_eps) * (kn.knn_fr[i] * prm.dbscan_eps);
    dv.knn_s = mc::knn_scale(dv.eps2);
    dv.ce = prm.dbscan_eps * 1.01;
    dv.frac = prm.component_min_fraction;
    dv.std_ratio = prm.sor_std_ratio;
    dv.cov = prm.coverage_threshold;
    dv.r2 = rf * rf;
    dv.scene_inv = 1.0f / (2.0f * rf);
    dv.minpts = prm.dbscan_min_points;
    dv.knn = prm.sor_neighbors;
    dv.kball = prm.ball_k;
    dv.few = prm.few_points;
    dv.H = H;
    dv.W = W;
    dv.nbands = nbands;
    dv.nbcap = kn.nbcap;
    dv.vec4 = (W % 4 == 0 && reinterpret_cast<uintptr_t>(dep) % 16 == 0 && reinterpret_cast<uintptr_t>(sg) % 4 == 0)
                  ? 1 : 0;
    return dv;
}

// ---- one batch: frames [b0, b0 + fb) of the call ----
struct BpBatch {
    int b0, fb;
    const float *dB;    // the batch's depth / seg frames, intrinsics and poses (device)
    const uint8_t *sB;
    const double *KB, *TB;
    int *st;            // the device status block (BpStat)
    const mc::BpDev &dv;
    int ncap, nslot;    // slot-list stride of the batch (slots_cap(fb)); its (frame, id) slots
    int fb_cap;         // frames per batch the arrays are laid out for
};

int bp_px_cap_int(const BpState &bp) { return static_cast<int>(std::min<size_t>(bp.px_cap, INT_MAX)); }

// The k-NN ring search (k_bp_knn_ring) and the statistics / survivors (k_bp_denoise_tail) of every LDS
// class, once after the classes join, over one queue (queued per class behind each class kernel they
// measured 2 % slower at C3: the concurrent ring searches competed with the remaining classes,
// profiles/r04/r4e_tail_ab.jsonl)
void bp_denoise_tail_launch(mc_ctx *ctx, hipStream_t s, const BpBatch &bt, int tail_wg)
{
    BpState &bp = ctx->bp;
    int *st = bt.st;
    // eight workgroups per CU (four waves per SIMD; at five or six, spilling: no faster)
    hipLaunchKernelGGL(mc::k_bp_knn_ring<4>, dim3(ctx->num_cu * 8), dim3(256), 0, s, st + BS_DQ, bp.vx_pvid.as<int>(),
                       bp.slot_pix.as<int>(), bp.slot_m.as<int>(), bt.dv, bp.acc.as<double4>(), bp.bstart.as<int>(),
                       bp.vx_list.as<int>(), bp.slot_grid.as<double>(), bp.avg.as<double>(), st + BS_DNERR);
    // a wave per slot whose ordered sums wait on latency: as many waves as its 45 VGPRs allow
    hipLaunchKernelGGL(mc::k_bp_denoise_tail, dim3(ctx->num_cu * tail_wg), dim3(256), 0, s, st + BS_CLS,
                       bp.cls_list.as<int>(), bt.ncap, 0, mc::kBpClasses, bp.slot_pix.as<int>(), bp.slot_m.as<int>(),
                       bt.dv, bp.vpts.as<double>(), bp.avg.as<double>(), bp.ssidx.as<int>(), bp.qpts.as<float>(),
                       bp.slot_ns.as<int>(), bp.slot_box.as<float>());
}

// one LDS size class of the denoise: as many workgroups as are resident at once (times kBpOversub),
// each taking the class's slots from a ticket counter
template <int N>
void bp_denoise_class(mc_ctx *ctx, hipStream_t s, const BpBatch &bt)
{
    using C = mc::BpLdsClass<N>;
    constexpr int cls = bp_class_index(N);
    static_assert(cls >= 0, "not an LDS size class");
    BpState &bp = ctx->bp;
    int *st = bt.st;
    // the classes run concurrently: each has its own region of per-workgroup neighbour lists
    hipLaunchKernelGGL(mc::k_bp_denoise_lds<N>, dim3(ctx->num_cu * C::kWgPerCu * kBpOversub), dim3(C::T), 0, s,
                       st + BS_CLS + cls, bp.cls_list.as<int>() + static_cast<size_t>(cls) * bt.ncap, st + BS_TK + cls,
                       bp.slot_pix.as<int>(), bp.slot_nv.as<int>(), bt.dv, bp.vpts.as<double>(),
                       bp.nbl.as<unsigned short>() + nbl_offset(ctx, cls), bp.lean.as<int>() + lean_offset(ctx, cls),
                       bp.slot_m.as<int>(), bp.avg.as<double>(), bp.ssidx.as<int>(), bp.acc.as<double4>(),
                       bp.bstart.as<int>(), bp.vx_list.as<int>(), bp.vx_pvid.as<int>(), st + BS_DQ, bp_px_cap_int(bp),
                       bp.slot_grid.as<double>(), st + BS_DNERR);
}

// valid pixels per (frame, id), the candidate slots and their pixel lists
void bp_launch_pixels(mc_ctx *ctx, hipStream_t s, const BpBatch &bt)
{
    BpState &bp = ctx->bp;
    int *st = bt.st;
    const int fb = bt.fb, nslot = bt.nslot, nbands = bt.dv.nbands;
    TimedScope ts(ctx->timer, s, "bp_pixels");
    hipLaunchKernelGGL(mc::k_bp_stat_init, dim3(1), dim3(64), 0, s, st, static_cast<int>(BS_COUNT));
    MC_HIP(hipMemsetAsync(bp.present.ptr, 0, fb * 8 * 4, s));
    MC_HIP(hipMemsetAsync(bp.fflags.ptr, 0, fb * 4, s));
    hipLaunchKernelGGL(mc::k_bp_count, dim3(nbands, fb), dim3(256), 0, s, bt.dB, bt.sB, bt.TB, bt.dv, bp.band.as<int>(),
                       bp.present.as<unsigned>(), bp.fflags.as<int>(), bp.vid.as<unsigned char>());
    hipLaunchKernelGGL(mc::k_bp_frames, dim3(fb), dim3(1024), 0, s, bp.band.as<int>(), bp.present.as<unsigned>(),
                       bp.fflags.as<int>(), bt.dv, bp.cand.as<int>(), bp.npix.as<int>(), st + BS_ERRF);
    mc::scan_device_multi(s, nullptr, nslot, bp.scanm.as<int>(), bp.cand.as<int>(), bp.csidx.as<int>(), st + BS_NS,
                          bp.npix.as<int>(), bp.poff.as<int>(), st + BS_NPX);
    hipLaunchKernelGGL(mc::k_bp_slots, grid_for(nslot), dim3(256), 0, s, bp.cand.as<int>(), bp.csidx.as<int>(),
                       bp.npix.as<int>(), bp.poff.as<int>(), nslot, bp.slot_of.as<int>(), bp.slot_frame.as<int>(),
                       bp.slot_id.as<int>(), bp.slot_np.as<int>(), bp.slot_pix.as<int>(), st + BS_NPX,
                       bp_px_cap_int(bp), st + BS_NS, st + BS_PXOVF);
    hipLaunchKernelGGL(mc::k_bp_compact, dim3(nbands, fb), dim3(256), 0, s, bp.vid.as<unsigned char>(),
                       bp.band.as<int>(), bp.slot_of.as<int>(), bp.slot_pix.as<int>(), bt.dv,
                       bp.pix_list.as<unsigned>());
    bp_debug_sync(s, "bp_pixels");
}

// voxel_down_sample: the first LDS tier, the larger one for the slots it hands on, the global hash
void bp_launch_voxel(mc_ctx *ctx, hipStream_t s, const BpBatch &bt, int vx_global)
{
    BpState &bp = ctx->bp;
    int *st = bt.st;
    TimedScope ts(ctx->timer, s, "bp_voxel");
    hipLaunchKernelGGL(mc::k_bp_vox_order, dim3(1), dim3(1024), 0, s, st + BS_NS, bp.slot_np.as<int>(),
                       bp.vox_order.as<int>());
    int *fb1 = bp.vx_fb.as<int>(), *fb2 = fb1 + slots_cap(bt.fb_cap);
    // five workgroups per CU (32 KB of LDS, <= 96 VGPRs each) for the first tier
    hipLaunchKernelGGL(HIP_KERNEL_NAME(mc::k_bp_voxel_lds<mc::kVxT, mc::kVxH, mc::kVxV, 0, mc::kVxWpe>),
                       dim3(ctx->num_cu * mc::kVxWpe), dim3(mc::kVxT), 0, s, st + BS_NS, bp.vox_order.as<int>(),
                       bp.slot_frame.as<int>(), bp.slot_np.as<int>(), bp.slot_pix.as<int>(), bp.pix_list.as<unsigned>(),
                       bt.dB, bt.KB, bt.TB, bt.dv, bp.vx_pvid.as<int>(), bp.vpts.as<double>(), bp.slot_nv.as<int>(), fb1,
                       st + BS_VXFB, vx_global >= 1 ? 1 : 0, bp.slot_grid.as<double>());
    hipLaunchKernelGGL(HIP_KERNEL_NAME(mc::k_bp_voxel_lds<mc::kVxT2, mc::kVxH2, mc::kVxV2, mc::kVxL2>), dim3(ctx->num_cu),
                       dim3(mc::kVxT2), 0, s, st + BS_VXFB, fb1, bp.slot_frame.as<int>(), bp.slot_np.as<int>(),
                       bp.slot_pix.as<int>(), bp.pix_list.as<unsigned>(), bt.dB, bt.KB, bt.TB, bt.dv, bp.vx_pvid.as<int>(),
                       bp.vpts.as<double>(), bp.slot_nv.as<int>(), fb2, st + BS_VXFB2, vx_global == 1 ? 1 : 0,
                       bp.slot_grid.as<double>());
    hipLaunchKernelGGL(mc::k_bp_voxel, dim3(ctx->num_cu), dim3(256), 0, s, st + BS_VXFB2, fb2, bp.slot_frame.as<int>(),
                       bp.slot_np.as<int>(), bp.slot_pix.as<int>(), bp.pix_list.as<unsigned>(), bt.dB, bt.KB, bt.TB, bt.dv,
                       bp.hkey.as<unsigned long long>(), bp.hvid.as<int>(), bp.hfirst.as<int>(), bp.vox_entry.as<int>(),
                       bp.acc.as<double>(), bp.vpts.as<double>(), bp.slot_nv.as<int>(), st + BS_VOXERR,
                       bp.slot_grid.as<double>());
    bp_debug_sync(s, "bp_voxel");
}

// DBSCAN, the component filter and the outlier removal of every slot, by size class
void bp_launch_denoise(mc_ctx *ctx, hipStream_t s, const BpBatch &bt, const BpKnobs &kn)
{
    BpState &bp = ctx->bp;
    int *st = bt.st;
    const int ncap = bt.ncap;
    TimedScope ts(ctx->timer, s, "bp_denoise");
    // largest first again, now by voxel count (the denoise's and the query's cost)
    hipLaunchKernelGGL(mc::k_bp_vox_order, dim3(1), dim3(1024), 0, s, st + BS_NS, bp.slot_nv.as<int>(),
                       bp.vox_order.as<int>());
    hipLaunchKernelGGL(mc::k_bp_classify, dim3(64), dim3(256), 0, s, st + BS_NS, bp.slot_nv.as<int>(),
                       bp.vox_order.as<int>(), ncap, kn.min_cls, st + BS_CLS, bp.cls_list.as<int>());
    // the few slots beyond the LDS classes run on the side stream, beside the classes
    MC_HIP(hipEventRecord(ctx->ev_fork, s));
    MC_HIP(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
    bp_denoise_class<16384>(ctx, ctx->side, bt);  // few, large slots
    hipLaunchKernelGGL(mc::k_bp_denoise, dim3(ctx->num_cu), dim3(256), 0, ctx->side, st + BS_CLS + mc::kBpClasses,
                       bp.cls_list.as<int>() + mc::kBpClasses * static_cast<size_t>(ncap), bp.slot_pix.as<int>(),
                       bp.slot_nv.as<int>(), bt.dv, bp.vpts.as<double>(), bp.pcell.as<unsigned long long>(),
                       bp.pbkt.as<int>(), bp.bcnt.as<int>(), bp.bstart.as<int>(), bp.blist.as<int>(), bp.ncnt.as<int>(),
                       bp.par.as<int>(), bp.droot.as<int>(), bp.rnk.as<int>(), bp.lab.as<int>(), bp.ccnt.as<int>(),
                       bp.ssidx.as<int>(), bp.avg.as<double>(), bp.qpts.as<float>(), bp.slot_m.as<int>(),
                       bp.slot_ns.as<int>(), bp.slot_box.as<float>());
    MC_HIP(hipEventRecord(ctx->ev_join, ctx->side));
    // the LDS classes side by side, each on its own stream: a class with few slots
    // (the large ones) leaves most CUs to the others instead of serialising the batch
    for (int c = 0; c < mc::kBpStreamClasses; c++) MC_HIP(hipStreamWaitEvent(bp.cls_stream[c], ctx->ev_fork, 0));
    bp_denoise_class<3072>(ctx, bp.cls_stream[bp_class_index(3072)], bt);
    bp_denoise_class<4096>(ctx, bp.cls_stream[bp_class_index(4096)], bt);
    bp_denoise_class<2048>(ctx, bp.cls_stream[bp_class_index(2048)], bt);
    bp_denoise_class<1024>(ctx, bp.cls_stream[bp_class_index(1024)], bt);
    bp_denoise_class<512>(ctx, bp.cls_stream[bp_class_index(512)], bt);
    for (int c = 0; c < mc::kBpStreamClasses; c++) {
        MC_HIP(hipEventRecord(bp.ev_cls[c], bp.cls_stream[c]));
        MC_HIP(hipStreamWaitEvent(s, bp.ev_cls[c], 0));
    }
    MC_HIP(hipStreamWaitEvent(s, ctx->ev_join, 0));
    // the deferred points' ring search, then every LDS-class slot's statistics and survivors
    bp_denoise_tail_launch(ctx, s, bt, kn.tail_wg);
    bp_debug_sync(s, "bp_denoise");
}

// scene points within the ball radius of each slot's points (PW: words of a point bitmap; tmp_cap:
// ints of the neighbour-set pool), then the kept masks' indices and offsets
void bp_launch_query(mc_ctx *ctx, hipStream_t s, const BpBatch &bt, int PW, size_t tmp_cap, const BpKnobs &kn)
{
    BpState &bp = ctx->bp;
    int *st = bt.st;
    TimedScope ts(ctx->timer, s, "bp_query");
    const int tcap = static_cast<int>(std::min<size_t>(tmp_cap, INT_MAX));
    // the slots whose box cells and cropped scene points fit LDS (largest first); the rest go to q_fb
    hipLaunchKernelGGL(mc::k_bp_query_lds, dim3(kn.q_grid ? kn.q_grid : ctx->num_cu * kBpQueryLdsWgPerCu), dim3(256), 0, s,
                       st + BS_NS, bp.slot_pix.as<int>(), bp.slot_ns.as<int>(), bp.slot_box.as<float>(),
                       bp.qpts.as<float>(), bt.dv, bp.gpts.as<float4>(), bp.gcell.as<unsigned long long>(),
                       bp.gstart.as<int>(), bp.gnb, bp.tmp.as<int>(), tcap, st + BS_TOP, bp.slot_nn.as<int>(),
                       bp.slot_toff.as<int>(), bp.slot_cov.as<int>(), st + BS_OVF, bp.vox_order.as<int>(),
                       bp.kflag.as<int>(), bp.ksize.as<int>(), bp.q_fb.as<int>(), st + BS_QFB,
                       kn.q_staged ? kn.q_cells : 0, kn.q_cand);
    bp_debug_sync(s, "k_bp_query_lds");
    // k_bp_query over that list (few slots, the large ones: workgroups beyond its length end at once)
    auto query = [&](auto kern, int wg_per_cu) {
        const int grid = ctx->num_cu * wg_per_cu;
        MC_REQUIRE(static_cast<size_t>(grid) * PW * 8 <= bp.bm.bytes, MC_ERR_HIP,
                   "query grid beyond its point bitmaps (internal error)");
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, st + BS_QFB, bp.slot_pix.as<int>(), bp.slot_ns.as<int>(),
                           bp.slot_box.as<float>(), bp.qpts.as<float>(), bt.dv, bp.gpts.as<float4>(), bp.gidx.as<int>(),
                           bp.gcell.as<unsigned long long>(), bp.gstart.as<int>(), bp.gnb,
                           bp.bm.as<unsigned long long>(), PW, bp.tmp.as<int>(), tcap, st + BS_TOP, bp.slot_nn.as<int>(),
                           bp.slot_toff.as<int>(), bp.slot_cov.as<int>(), st + BS_OVF, bp.q_fb.as<int>(),
                           bp.kflag.as<int>(), bp.ksize.as<int>());
    };
    if (bt.dv.kball <= 20) query(mc::k_bp_query<1, 20>, kBpQueryWgPerCu20);
    else query(mc::k_bp_query<1, mc::kBpBallMax>, kBpQueryWgPerCu32);
    bp_debug_sync(s, "k_bp_query");
    mc::scan_device_multi(s, st + BS_NS, bt.nslot, bp.scanm.as<int>(), bp.kflag.as<int>(), bp.midx.as<int>(), st + BS_M,
                          bp.ksize.as<int>(), bp.moff.as<int>(), st + BS_NNZ);
    bp_debug_sync(s, "bp_query");
}

// What a batch's status block (hs: its pinned copy) asks for.  Input and internal errors throw.
enum class BpVerdict { kOk, kRedoPixels, kRedoNeighbours };

BpVerdict bp_check_batch(mc_ctx *ctx, const int *hs, int b0)
{
    if (hs[BS_ERRF] != INT_MAX) {
        ctx->bp.err_frame = b0 + hs[BS_ERRF];
        throw McError{MC_ERR_INVALID, "frame " + std::to_string(b0 + hs[BS_ERRF]) +
                                          ": depth pixel equal to depth_trunc (the reference raises "
                                          "IndexError at utils/mask_backprojection.py:100)"};
    }
    MC_REQUIRE(!(hs[BS_VOXERR] & 2), MC_ERR_HIP, "voxel hash table not empty at slot start (internal error)");
    MC_REQUIRE(hs[BS_DNERR] == 0, MC_ERR_HIP,
               "denoise: k-NN ring-search queue " + std::string(hs[BS_DNERR] & 1 ? "entry" : "region") +
                   " out of range (internal error)");
    MC_REQUIRE(hs[BS_VOXERR] == 0, MC_ERR_UNSUPPORTED, "voxel index beyond 2^21 per axis");
    if (hs[BS_PXOVF]) return BpVerdict::kRedoPixels;  // more mask pixels than the capacity: nothing past the pixel lists ran
    if (hs[BS_OVF]) return BpVerdict::kRedoNeighbours;  // the neighbour sets overflowed tmp
    return BpVerdict::kOk;
}

// The host side of a batch (its masks and statistics appended from h_pack) runs while the next batch
// computes: the batch's copy into h_pack is stream-ordered before the next batch, whose own copy
// comes only after its statistics sync, i.e. after this append
struct BpPending {
    bool valid = false;
    int b0 = 0, Mb = 0, NS = 0, nnzb = 0;
    int64_t nnz_base = 0;
    void append(BpState &bp, int few_points)
    {
        if (!valid) return;
        MC_HIP(hipEventSynchronize(bp.ev_pack));
        const int *col = bp.h_pack, *lab = col + Mb, *off = lab + Mb;
        const int *sf = off + Mb, *sid = sf + NS, *snp = sid + NS, *snv = snp + NS, *sm = snv + NS,
                  *sns = sm + NS, *scov = sns + NS, *snn = scov + NS;
        for (int g = 0; g < Mb; g++) {
            bp.col.push_back(b0 + col[g]);
            bp.label.push_back(lab[g]);
        }
        for (int g = 0; g < Mb; g++) bp.off.push_back(nnz_base + (g + 1 < Mb ? off[g + 1] : nnzb));
        for (int x = 0; x < NS; x++) {
            const int kept = snn[x] >= 0;
            const int row[MC_BP_NSTAT] = {b0 + sf[x], sid[x], snp[x], snv[x], sm[x], sns[x], -1,
                                          sns[x] >= few_points ? scov[x] : 0, kept ? snn[x] : 0, kept};
            bp.stats.insert(bp.stats.end(), row, row + MC_BP_NSTAT);
        }
        valid = false;
    }
};

// the batch's kept masks: their point lists appended to bp.pts; their (col, label, off) and the 8
// per-candidate statistics arrays packed on the device, one copy into pinned memory
BpPending bp_emit_pack(mc_ctx *ctx, hipStream_t s, const BpBatch &bt, const int *hs)
{
    BpState &bp = ctx->bp;
    int *st = bt.st;
    const int NS = hs[BS_NS], Mb = hs[BS_M], nnzb = hs[BS_NNZ];
    bp.out_col.reserve((Mb + 1) * 4);
    bp.out_label.reserve((Mb + 1) * 4);
    bp.out_off.reserve((Mb + 1) * 4);
    grow_keep(bp.pts, (bp.nnz + nnzb + 1) * 4, bp.nnz * 4, s);
    {
        TimedScope ts(ctx->timer, s, "bp_query");
        hipLaunchKernelGGL(mc::k_bp_emit, grid_for(std::max(NS, 1), 4, 4096), dim3(256), 0, s, st + BS_NS,
                           bp.slot_frame.as<int>(), bp.slot_id.as<int>(), bp.slot_nn.as<int>(), bp.slot_toff.as<int>(),
                           bp.midx.as<int>(), bp.moff.as<int>(), bp.tmp.as<int>(), bp.out_col.as<int>(),
                           bp.out_label.as<int>(), bp.out_off.as<int>(), bp.pts.as<int>() + bp.nnz);
    }
    const size_t npack = 3 * static_cast<size_t>(Mb) + 8 * static_cast<size_t>(NS);
    bp.pack.reserve((npack + 1) * 4);
    if (bp.h_pack_n < npack) {
        if (bp.h_pack) MC_HIP(hipHostFree(bp.h_pack));
        bp.h_pack = nullptr;
        bp.h_pack_n = 0;
        const size_t n = npack + npack / 2 + 1024;
        MC_HIP(hipHostMalloc(reinterpret_cast<void **>(&bp.h_pack), n * 4, hipHostMallocDefault));
        bp.h_pack_n = n;
    }
    if (npack) {
        hipLaunchKernelGGL(mc::k_bp_pack, grid_for(static_cast<int64_t>(npack)), dim3(256), 0, s, st + BS_NS, st + BS_M,
                           bp.out_col.as<int>(), bp.out_label.as<int>(), bp.out_off.as<int>(), bp.slot_frame.as<int>(),
                           bp.slot_id.as<int>(), bp.slot_np.as<int>(), bp.slot_nv.as<int>(), bp.slot_m.as<int>(),
                           bp.slot_ns.as<int>(), bp.slot_cov.as<int>(), bp.slot_nn.as<int>(), bp.pack.as<int>());
        MC_HIP(hipMemcpyAsync(bp.h_pack, bp.pack.ptr, npack * 4, hipMemcpyDeviceToHost, s));
    }
    MC_HIP(hipEventRecord(bp.ev_pack, s));
    bp_debug_sync(s, "bp_emit");
    bp.nnz += nnzb;
    return BpPending{true, bt.b0, Mb, NS, nnzb, bp.nnz - nnzb};
}

// the arguments every S1 entry shares; the call's parameters
mc_bp_params bp_validate(mc_ctx *ctx, int F, int H, int W, const BpFrames &src, const mc_bp_params *params)
{
    MC_REQUIRE(ctx->bp.have_points, MC_ERR_STATE, "mc_backproject before mc_scene_set_points");
    MC_REQUIRE(F >= 0 && H > 0 && W > 0, MC_ERR_INVALID, "bad frame sizes");
    MC_REQUIRE(F == 0 || src.given(F), MC_ERR_INVALID, "null frame arrays");
    MC_REQUIRE(static_cast<int64_t>(H) * W < (int64_t(1) << 31), MC_ERR_UNSUPPORTED, "image too large");
    mc_bp_params prm;
    if (params) prm = *params;
    else mc_bp_params_default(&prm);
    MC_REQUIRE(prm.sor_neighbors >= 1 && prm.sor_neighbors <= mc::kBpKnnMax, MC_ERR_UNSUPPORTED,
               "sor_neighbors must be in [1, 20]");
    MC_REQUIRE(prm.ball_k >= 1 && prm.ball_k <= mc::kBpBallMax, MC_ERR_UNSUPPORTED, "ball_k must be in [1, 32]");
    MC_REQUIRE(prm.voxel_size > 0 && prm.dbscan_eps > 0 && prm.ball_radius > 0, MC_ERR_INVALID, "bad radii");
    return prm;
}

// the call's buffers that do not depend on the batch: the query's point bitmaps and neighbour-set
// pool, the status block's pinned copy.  Returns the pool's capacity in ints.
size_t bp_reserve_call(mc_ctx *ctx, int PW, hipStream_t s)
{
    BpState &bp = ctx->bp;
    const size_t bm_bytes = static_cast<size_t>(ctx->num_cu) * kBpQueryWgPerCuMax * PW * 8;  // a bitmap per query workgroup
    if (bp.bm.bytes < bm_bytes) {
        bp.bm.reserve(bm_bytes);
        MC_HIP(hipMemsetAsync(bp.bm.ptr, 0, bp.bm.bytes, s));  // kept zero by k_bp_query
    }
    const size_t tmp_cap = std::max<size_t>(bp.tmp.bytes / 4, std::max<size_t>(1 << 20, bp.px_cap));
    bp.tmp.reserve(tmp_cap * 4);
    if (!bp.h_stat) MC_HIP(hipHostMalloc(reinterpret_cast<void **>(&bp.h_stat), BS_COUNT * sizeof(int), hipHostMallocDefault));
    if (!bp.ev_pack) MC_HIP(hipEventCreateWithFlags(&bp.ev_pack, hipEventDisableTiming));
    return tmp_cap;
}

// S1 for F frames of H x W from src; the results stay in ctx->bp (mc_backproject_get_*)
void bp_run(mc_ctx *ctx, int F, int H, int W, BpFrames src, const mc_bp_params *params)
{
    BpState &bp = ctx->bp;
    const mc_bp_params prm = bp_validate(ctx, F, H, W, src, params);
    const BpKnobs kn = bp_read_knobs(ctx);
    hipStream_t s = ctx->stream;
    const size_t HW = static_cast<size_t>(H) * W;
    const int nbands = (H + mc::kBpBand - 1) / mc::kBpBand;
    bp.have_result = false;
    bp.F = F;
    bp.err_frame = -1;
    bp.col.clear(), bp.label.clear(), bp.stats.clear();
    bp.off.assign(1, 0);
    bp.nnz = 0;
    bp.batches = 0;
    const float rf = static_cast<float>(prm.ball_radius);
    if (bp.grid_radius != rf) {  // a new scene (mc_scene_set_points) or radius: the 2r scene grid
        TimedScope ts(ctx->timer, s, "bp_grid");
        bp_build_grid(ctx, rf, s);
    }
    bp_bind_frames(ctx, src, F, HW, s);

    // the batch plan (mc_bp_plan.hpp)
    const bool staged = src.kind == BpFrames::kHostFrames && F;
    const double mfrac = std::min(1.0, std::max(bp.mfrac, 1e-4));
    size_t free_b = 0, total_b = 0;
    if (bp.mem_budget <= 0 && hipMemGetInfo(&free_b, &total_b) != hipSuccess) total_b = 0;
    const size_t bud_bytes = mc::bp_byte_budget(bp.mem_budget, free_b, total_b, mc::bp_held_bytes(bp.px_cap, bp.fpx_cap));
    const size_t budget = kn.fixed_batch ? kn.batch_pixels : mc::bp_pixel_budget(bud_bytes, mfrac, HW);
    int FB = mc::bp_frames_per_batch(F, HW, budget, staged ? kn.upload_batches : 0);
    bp_reserve(ctx, FB, H, W, nbands, mc::bp_mask_cap(FB, HW, mfrac), s);
    const int PW = static_cast<int>((bp.P + 63) / 64) + 1;
    size_t tmp_cap = bp_reserve_call(ctx, PW, s);
    const mc::BpDev dv = bp_make_dev(prm, kn, H, W, nbands, src.depth, src.seg);
    int *const st = bp.stat.as<int>();
    int *const hs = bp.h_stat;  // pinned
    double mfrac_seen = 0.0;
    BpPending pend;
    for (int b0 = 0; b0 < F;) {
        const int fb = std::min(FB, F - b0);
        if (staged) {
            bp_stage_to(ctx, src, b0 + fb, H, W, kn.stage_threads);
            MC_HIP(hipStreamWaitEvent(s, bp.ev_up, 0));
        }
        const BpBatch bt{b0, fb, src.depth + b0 * HW, src.seg + b0 * HW, src.intr + 4 * static_cast<size_t>(b0),
                         src.pose + 16 * static_cast<size_t>(b0), st, dv, static_cast<int>(slots_cap(fb)), fb * 256, FB};
        bp_launch_pixels(ctx, s, bt);
        bp_launch_voxel(ctx, s, bt, kn.vx_global);
        bp_launch_denoise(ctx, s, bt, kn);
        bp_launch_query(ctx, s, bt, PW, tmp_cap, kn);
        MC_HIP(hipMemcpyAsync(hs, st, BS_COUNT * 4, hipMemcpyDeviceToHost, s));
        bp_stage_to(ctx, src, std::min(F, b0 + fb + FB), H, W, kn.stage_threads);  // the host copies the next batch while this one computes
        pend.append(bp, prm.few_points);                                           // and appends the previous batch's results
        MC_HIP(hipStreamSynchronize(s));
        ctx->timer.collect();
        const BpVerdict v = bp_check_batch(ctx, hs, b0);
        if (kn.q_report)
            fprintf(stderr, "[mc bp] batch at frame %d: %d slots, %d took k_bp_query\n", b0, hs[BS_NS], hs[BS_QFB]);
        const double frac = static_cast<double>(hs[BS_NPX]) / (static_cast<double>(fb) * HW);
        if (v == BpVerdict::kRedoPixels) {  // grow to the share the batch showed, or take fewer frames, and redo it
            bp.mfrac = std::max(bp.mfrac, frac);
            const int fb_was = FB;
            FB = mc::bp_shrink_after_overflow(FB, HW, frac, bud_bytes, kn.fixed_batch);
            bp_reserve(ctx, FB, H, W, nbands, mc::bp_redo_mask_cap(FB, fb_was, HW, frac, static_cast<size_t>(hs[BS_NPX])), s);
            bp.redo++;
            continue;
        }
        mfrac_seen = std::max(mfrac_seen, frac);
        if (v == BpVerdict::kRedoNeighbours) {  // grow the neighbour-set pool and redo the batch
            tmp_cap = static_cast<size_t>(hs[BS_TOP]) + (static_cast<size_t>(hs[BS_TOP]) >> 1) + 1024;
            bp.tmp.reserve(tmp_cap * 4);
            continue;
        }
        bp.batches++;
        bp.vx_handed[0] = hs[BS_VXFB];
        bp.vx_handed[1] = hs[BS_VXFB2];
        pend = bp_emit_pack(ctx, s, bt, hs);
        b0 += fb;
    }
    // the next call's batches are sized for the share seen, decaying from the larger of earlier calls
    // (a stream of scenes on one context: a sparse scene does not at once size batches a denser one
    // after it overflows)
    if (mfrac_seen > 0.0) {
        bp.mfrac = bp.mfrac_obs ? std::max(mfrac_seen, 0.5 * (bp.mfrac + mfrac_seen)) : mfrac_seen;
        bp.mfrac_obs = true;
    }
    bp.last_fb = FB;
    pend.append(bp, prm.few_points);
    MC_HIP(hipStreamSynchronize(s));
    bp.have_result = true;
}

// mc_backproject_frames / _raw: per-frame host arrays, staged by bp_run's batch loop itself
int backproject_frames_impl(mc_ctx *ctx, int32_t num_frames, int32_t height, int32_t width,
                            const void *const *depth_frames, double raw_scale, const uint8_t *const *seg_frames,
                            const double *intrinsics, const double *poses, const mc_bp_params *params)
{
    const int rc = guarded(ctx, [&] {
        MC_REQUIRE(raw_scale >= 0.0 && std::isfinite(raw_scale), MC_ERR_INVALID, "bad depth_scale");
        const BpFrames src{BpFrames::kHostFrames, nullptr, nullptr, depth_frames,
                           reinterpret_cast<const void *const *>(seg_frames), intrinsics, poses, raw_scale};
        bp_run(ctx, num_frames, height, width, src, params);
    });
    if (ctx && ctx->bp.copy) (void)hipStreamSynchronize(ctx->bp.copy);  // no DMA into in_* outlives the call (error paths)
    return rc;
}

}  // namespace

extern "C" {

void mc_bp_params_default(mc_bp_params *p)
{
    if (!p) return;
    p->depth_trunc = 20.0;
    p->voxel_size = 0.01;
    p->dbscan_eps = 0.04;
    p->component_min_fraction = 0.2;
    p->sor_std_ratio = 2.0;
    p->ball_radius = 0.01;
    p->coverage_threshold = 0.3;
    p->dbscan_min_points = 4;
    p->sor_neighbors = 20;
    p->ball_k = 20;
    p->few_points = 25;
}

int mc_scene_set_points(mc_ctx *ctx, int64_t num_points, const float *xyz, int on_device)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(num_points >= 0 && num_points < (int64_t(1) << 31) - 1, MC_ERR_UNSUPPORTED, "num_points out of range");
        MC_REQUIRE(num_points == 0 || xyz, MC_ERR_INVALID, "null points");
        hipStream_t s = ctx->stream;
        BpState &bp = ctx->bp;
        bp.P = num_points;
        bp.scene.reserve((num_points + 1) * 12);
        if (num_points)
            MC_HIP(hipMemcpyAsync(bp.scene.ptr, xyz, num_points * 12,
                                  on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
        bp.have_points = true;
        bp.have_result = false;
        bp.grid_radius = -1.f;  // the grid is built by the next mc_backproject
        MC_HIP(hipStreamSynchronize(s));
    });
}

int mc_backproject_frames(mc_ctx *ctx, int32_t num_frames, int32_t height, int32_t width,
                          const float *const *depth_frames, const uint8_t *const *seg_frames,
                          const double *intrinsics, const double *poses, const mc_bp_params *params)
{
    return backproject_frames_impl(ctx, num_frames, height, width, reinterpret_cast<const void *const *>(depth_frames),
                                   0.0, seg_frames, intrinsics, poses, params);
}

int mc_backproject_frames_raw(mc_ctx *ctx, int32_t num_frames, int32_t height, int32_t width,
                              const uint16_t *const *depth_frames, double depth_scale,
                              const uint8_t *const *seg_frames, const double *intrinsics, const double *poses,
                              const mc_bp_params *params)
{
    if (!(depth_scale > 0.0)) return guarded(ctx, [&] { MC_REQUIRE(false, MC_ERR_INVALID, "depth_scale must be > 0"); });
    return backproject_frames_impl(ctx, num_frames, height, width, reinterpret_cast<const void *const *>(depth_frames),
                                   depth_scale, seg_frames, intrinsics, poses, params);
}

int mc_backproject(mc_ctx *ctx, int32_t num_frames, int32_t height, int32_t width, const float *depth,
                   const uint8_t *seg, const double *intrinsics, const double *poses, int on_device,
                   const mc_bp_params *params)
{
    return guarded(ctx, [&] {
        const BpFrames src{on_device ? BpFrames::kDevice : BpFrames::kHost, depth, seg, nullptr, nullptr, intrinsics, poses};
        bp_run(ctx, num_frames, height, width, src, params);
    });
}

int mc_backproject_get_info(mc_ctx *ctx, mc_bp_info *info)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(info, MC_ERR_INVALID, "null info");
        info->num_frames = ctx->bp.F;
        info->num_candidates = static_cast<int32_t>(ctx->bp.stats.size() / MC_BP_NSTAT);
        info->num_masks = static_cast<int32_t>(ctx->bp.col.size());
        info->error_frame = ctx->bp.err_frame;
        info->num_mask_points = ctx->bp.nnz;
    });
}

int mc_backproject_get_batching(mc_ctx *ctx, int64_t *out4)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(out4, MC_ERR_INVALID, "null output");
        out4[0] = ctx->bp.last_fb;
        out4[1] = static_cast<int64_t>(ctx->bp.px_cap);
        out4[2] = static_cast<int64_t>(mc::bp_held_bytes(ctx->bp.px_cap, ctx->bp.fpx_cap));
        out4[3] = ctx->bp.redo;
    });
}

int mc_backproject_get_masks(mc_ctx *ctx, int32_t *mask_col, int32_t *mask_label, int64_t *mask_off,
                             int32_t *mask_pts)
{
    return guarded(ctx, [&] {
        const BpState &bp = ctx->bp;
        MC_REQUIRE(bp.have_result, MC_ERR_STATE, "no back-projection result");
        const size_t M = bp.col.size();
        if (mask_col) std::copy(bp.col.begin(), bp.col.end(), mask_col);
        if (mask_label) std::copy(bp.label.begin(), bp.label.end(), mask_label);
        if (mask_off) std::copy(bp.off.begin(), bp.off.begin() + M + 1, mask_off);
        if (mask_pts && bp.nnz)
            MC_HIP(hipMemcpyAsync(mask_pts, bp.pts.ptr, bp.nnz * 4, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipStreamSynchronize(ctx->stream));
    });
}

int mc_backproject_copy_points_device(mc_ctx *ctx, int32_t *mask_pts_dev)
{
    return guarded(ctx, [&] {
        const BpState &bp = ctx->bp;
        MC_REQUIRE(bp.have_result, MC_ERR_STATE, "no back-projection result");
        MC_REQUIRE(mask_pts_dev || !bp.nnz, MC_ERR_INVALID, "null destination");
        if (bp.nnz)
            MC_HIP(hipMemcpyAsync(mask_pts_dev, bp.pts.ptr, bp.nnz * 4, hipMemcpyDeviceToDevice, ctx->stream));
    });
}

int mc_backproject_get_candidates(mc_ctx *ctx, int32_t *stats)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->bp.have_result, MC_ERR_STATE, "no back-projection result");
        std::copy(ctx->bp.stats.begin(), ctx->bp.stats.end(), stats);
    });
}

int mc_backproject_get_voxels(mc_ctx *ctx, int64_t *sizes3, int32_t *slots, uint32_t *pixels, double *means,
                              double *origins, int32_t *handed2)
{
    return guarded(ctx, [&] {
        const BpState &bp = ctx->bp;
        MC_REQUIRE(bp.have_result, MC_ERR_STATE, "no back-projection result");
        MC_REQUIRE(bp.batches == 1, MC_ERR_STATE,
                   "the voxel stage's arrays hold one batch: the last call ran " + std::to_string(bp.batches) +
                       " batches (mc_backproject_get_voxels needs exactly one)");
        MC_REQUIRE(sizes3, MC_ERR_INVALID, "null sizes");
        hipStream_t s = ctx->stream;
        // the slots of the batch are the call's candidates, in their order (frame, then id)
        const size_t NS = bp.stats.size() / MC_BP_NSTAT;
        std::vector<int32_t> sp(NS + 1, 0), snv(NS + 1, 0);
        if (NS) {
            MC_HIP(hipMemcpyAsync(sp.data(), bp.slot_pix.ptr, NS * 4, hipMemcpyDeviceToHost, s));
            MC_HIP(hipMemcpyAsync(snv.data(), bp.slot_nv.ptr, NS * 4, hipMemcpyDeviceToHost, s));
            MC_HIP(hipStreamSynchronize(s));
        }
        size_t npx = 0, nvx = 0, span = 0;  // span: pixel-list positions the slots' ranges reach
        for (size_t x = 0; x < NS; x++) {
            const int32_t *row = bp.stats.data() + x * MC_BP_NSTAT;
            MC_REQUIRE(sp[x] >= 0 && row[2] >= 0 && static_cast<size_t>(sp[x]) + row[2] <= bp.px_cap && snv[x] == row[3] &&
                           snv[x] <= row[2],
                       MC_ERR_HIP, "slot arrays differ from the call's candidates (internal error)");
            npx += row[2];
            nvx += snv[x];
            span = std::max(span, static_cast<size_t>(sp[x]) + row[2]);
        }
        sizes3[0] = static_cast<int64_t>(NS);
        sizes3[1] = static_cast<int64_t>(npx);
        sizes3[2] = static_cast<int64_t>(nvx);
        if (handed2) {
            handed2[0] = bp.vx_handed[0];
            handed2[1] = bp.vx_handed[1];
        }
        for (size_t x = 0; slots && x < NS; x++) {
            const int32_t *row = bp.stats.data() + x * MC_BP_NSTAT;
            const int32_t out[4] = {row[0], row[1], row[2], row[3]};
            std::copy(out, out + 4, slots + 4 * x);
        }
        if (!NS) return;
        if (pixels) {
            std::vector<uint32_t> pl(span + 1);
            MC_HIP(hipMemcpyAsync(pl.data(), bp.pix_list.ptr, span * 4, hipMemcpyDeviceToHost, s));
            MC_HIP(hipStreamSynchronize(s));
            for (size_t x = 0, o = 0; x < NS; o += bp.stats[x * MC_BP_NSTAT + 2], x++)
                std::copy(pl.begin() + sp[x], pl.begin() + sp[x] + bp.stats[x * MC_BP_NSTAT + 2], pixels + o);
        }
        if (means) {
            std::vector<double> vp(3 * span + 1);
            MC_HIP(hipMemcpyAsync(vp.data(), bp.vpts.ptr, 3 * span * 8, hipMemcpyDeviceToHost, s));
            MC_HIP(hipStreamSynchronize(s));
            for (size_t x = 0, o = 0; x < NS; o += snv[x], x++)
                std::copy(vp.begin() + 3 * static_cast<size_t>(sp[x]), vp.begin() + 3 * (static_cast<size_t>(sp[x]) + snv[x]),
                          means + 3 * o);
        }
        if (origins) {
            std::vector<double> sg(8 * NS);
            MC_HIP(hipMemcpyAsync(sg.data(), bp.slot_grid.ptr, 8 * NS * 8, hipMemcpyDeviceToHost, s));
            MC_HIP(hipStreamSynchronize(s));
            for (size_t x = 0; x < NS; x++) std::copy(sg.begin() + 8 * x, sg.begin() + 8 * x + 3, origins + 3 * x);
        }
    });
}

#ifdef MC_BP_STAMPS
// diagnostic builds only: read (and clear) k_bp_denoise's per-step clock totals
int mc_debug_bp_slot_times(unsigned *out, int n)
{
    n = std::min(n, 1 << 16);
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(mc::g_bp_slot_time), n * 4) == hipSuccess ? MC_OK : MC_ERR_HIP;
}
int mc_debug_bp_stamps(unsigned long long *out32)
{
    if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(mc::g_bp_stamps), 48 * 8) != hipSuccess) return MC_ERR_HIP;
    static const unsigned long long zero[48] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(mc::g_bp_stamps), zero, 48 * 8) == hipSuccess ? MC_OK : MC_ERR_HIP;
}
#endif

int mc_scene_use_backprojection(mc_ctx *ctx)
{
    if (!ctx) return MC_ERR_INVALID;
    if (!ctx->bp.have_result) {
        ctx->err = "no back-projection result";
        return MC_ERR_STATE;
    }
    const std::vector<int32_t> col = ctx->bp.col, lab = ctx->bp.label;
    const std::vector<int64_t> off = ctx->bp.off;
    return mc_scene_set_masks(ctx, ctx->bp.P, ctx->bp.F, static_cast<int32_t>(col.size()), col.data(), lab.data(),
                              off.data(), ctx->bp.pts.as<int32_t>(), 1);
}

}  // extern "C"
