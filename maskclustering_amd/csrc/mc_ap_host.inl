// mc_ap_host.inl — host side of the AP evaluation (mc_ev_*, include/mcgraph.h); kernels in
// mc_ap_kernels.inl.  Included by mc_api.hip after mc_pp_host.inl, whose pp_build_export it calls.
// What the host decides without the GPU is mc_ap_plan.hpp: no function here that launches a kernel
// checks a host table or parses buffer bytes.
//
// A scan reaches the accumulation in two halves.  mc_ev_add_scan* turn ground-truth ids and point
// lists into the scan's compact tables on the device (instances, kept predictions, non-zero
// same-class intersections) and fetch them: O(instances + predictions + pairs) words.  ev_commit()
// (shared with mc_ev_add_matches) checks the tables, lays them out per class, uploads them and runs
// the greedy pass, which appends (score, true) examples to per-(scan, class, overlap) regions whose
// sizes are known beforehand.  All checks come before the first write to the accumulation.
//
// mc_ev_state_*: the accumulation as a state buffer (per cell the distinct scores with their true /
// false counts, hard false negatives, flags).  ev_runs() builds it on the device from the same cell
// segments the table is computed from and keeps it until the accumulation changes; ev_merge() checks
// a buffer (header and per-cell sections on the host, the runs in a kernel) and appends its examples
// as one unit per non-empty cell.

namespace {

// grow a device array that holds `used` live bytes
void ev_grow(DevBuf &b, size_t used, size_t need, hipStream_t s)
{
    if (need <= b.bytes) return;
    DevBuf n;
    n.reserve(std::max(need, b.bytes * 2));
    if (used) MC_HIP(hipMemcpyAsync(n.ptr, b.ptr, used, hipMemcpyDeviceToDevice, s));
    MC_HIP(hipStreamSynchronize(s));
    b.swap(n);
}

// a message of mc_ap_plan.hpp as this call's error
void ev_require(const char *msg, int code)
{
    if (msg) throw McError{code, msg};
}

// room for `add` more examples in U more units
void ev_reserve_append(EvState &ev, int64_t add, int U, hipStream_t s)
{
    ev_grow(ev.d_ex_key, ev.ex_used * 8, (ev.ex_used + add) * 8 + 8, s);
    ev_grow(ev.d_ex_true, ev.ex_used, ev.ex_used + add + 8, s);
    ev_grow(ev.d_unit_cell, static_cast<size_t>(ev.units) * 4, static_cast<size_t>(ev.units + U) * 4 + 8, s);
    ev_grow(ev.d_unit_cnt, static_cast<size_t>(ev.units) * 4, static_cast<size_t>(ev.units + U) * 4 + 8, s);
    ev_grow(ev.d_unit_off, static_cast<size_t>(ev.units) * 8, static_cast<size_t>(ev.units + U) * 8 + 8, s);
}

// the planned scan's words to the device and the greedy pass over them (launches only)
void ev_greedy_pass(mc_ctx *ctx, const EvTables &t, const mc::EvScanPlan &p)
{
    EvState &ev = ctx->ev;
    hipStream_t s = ctx->stream;
    const int G = static_cast<int>(t.gcls.size()), K = static_cast<int>(t.pcls.size()), A = p.A, O = ev.O;
    const int64_t NP = static_cast<int64_t>(t.ppred.size());
    const size_t words = p.words.size() - 1;
    ev.d_words.reserve(words * 8 + 8);
    MC_HIP(hipMemcpyAsync(ev.d_words.ptr, p.words.data(), words * 8, hipMemcpyHostToDevice, s));
    const size_t b_q = static_cast<size_t>(NP) * 4, b_f = static_cast<size_t>(K) * 4, b_i = static_cast<size_t>(K) * 8,
                 b_v = static_cast<size_t>(O) * K;
    const size_t o_i = 0, o_q = o_i + b_i, o_f = o_q + ((b_q + 7) & ~size_t(7)), o_v = o_f + ((b_f + 7) & ~size_t(7));
    ev.d_tmp.reserve(o_v + b_v + 8);
    MC_HIP(hipMemsetAsync(ev.d_tmp.ptr, 0, o_v + b_v + 8, s));
    const mc::EvWords<const int64_t> w = mc::ev_words(ev.d_words.as<const int64_t>(), G, K, NP, A);
    char *T = ev.d_tmp.as<char>();
    mc::EvScanDev d{};
    d.G = G, d.K = K, d.NP = static_cast<int>(NP), d.A = A, d.O = O;
    d.min_region = ev.min_region;
    d.gvert = w.gvert, d.gid = w.gid, d.pvert = w.pvert, d.pvoid = w.pvoid, d.pslot = w.pslot;
    d.pscore = reinterpret_cast<const double *>(w.pscore);
    d.q_gt = w.q_gt, d.q_pred = w.q_pred, d.q_int = w.q_int;
    d.s_p0 = w.s_p0, d.s_p1 = w.s_p1, d.s_nfilt = w.s_nfilt, d.s_npred = w.s_npred, d.s_cls = w.s_cls;
    d.s_exoff = w.s_exoff, d.s_cap = w.s_cap;
    d.overlaps = ev.d_overlaps.as<double>();
    d.ign = reinterpret_cast<unsigned long long *>(T + o_i);
    d.qmask = reinterpret_cast<unsigned *>(T + o_q);
    d.found = reinterpret_cast<unsigned *>(T + o_f);
    d.visited = reinterpret_cast<unsigned char *>(T + o_v);
    d.ex_base = ev.ex_used, d.unit_base = ev.units;
    d.ex_key = ev.d_ex_key.as<unsigned long long>(), d.ex_true = ev.d_ex_true.as<unsigned char>();
    d.unit_cell = ev.d_unit_cell.as<int>(), d.unit_cnt = ev.d_unit_cnt.as<int>(), d.unit_off = ev.d_unit_off.as<int64_t>();
    d.cell_hardfn = ev.d_hardfn.as<unsigned long long>(), d.cell_flags = ev.d_flags.as<unsigned>();
    TimedScope ts(ctx->timer, s, "ev_greedy");
    if (NP) hipLaunchKernelGGL(mc::k_ev_qual, grid_for(NP), dim3(256), 0, s, d);
    hipLaunchKernelGGL(mc::k_ev_greedy, dim3(ceil_div(p.U, 4)), dim3(256), 0, s, d);
    if (K) hipLaunchKernelGGL(mc::k_ev_fp, grid_for(static_cast<int64_t>(K) * O), dim3(256), 0, s, d);
    MC_HIP(hipGetLastError());
}

void ev_commit(mc_ctx *ctx, EvTables &&t)
{
    EvState &ev = ctx->ev;
    hipStream_t s = ctx->stream;
    std::vector<int64_t> gt_poff;
    ev_require(mc::ev_check_tables(t, ev.C, gt_poff), MC_ERR_INVALID);
    const mc::EvScanPlan p = mc::ev_plan_scan(t, gt_poff, ev.C, ev.O, ev.min_region);
    ev_require(mc::ev_check_append(ev.ex_used, ev.units, static_cast<unsigned long long>(p.total), p.U), MC_ERR_UNSUPPORTED);
    // ---- from here on the accumulation changes ----
    ev_reserve_append(ev, p.total, p.U, s);
    if (p.A) ev_greedy_pass(ctx, t, p);
    MC_HIP(hipStreamSynchronize(s));  // the upload reads this call's host words
    ctx->timer.collect();
    ev.ex_used += p.total;
    ev.units += p.U;
    ev.last = std::move(t);
    ev.have_last = true;
    ev.ap_valid = false;
    ev.runs_valid = false;
}

// ---- the device half of mc_ev_add_scan*: every pointer is a device pointer -----------------------
struct EvScanIn {
    int64_t P;  // points, with their ground-truth ids
    const int *gt;
    int K;  // predictions as point lists (CSR, npts entries), classes and scores (either may be null)
    const int64_t *off;
    int64_t npts;
    const int *pts, *pcls;
    const double *pscore;
};

struct EvScanScratch {  // the pieces of d_pk (per prediction: keep, class, pairs, kept-before, pairs-before, vert, void) and d_class
    int *keep, *pcls, *npair, *kept, *pbase;
    int64_t *pvert, *pvoid;
    int *class_cnt, *class_first, *class_off;
};

// the inputs' ranges on the device; returns R, one more than the largest ground-truth id
int ev_scan_validate(mc_ctx *ctx, const EvScanIn &in)
{
    EvState &ev = ctx->ev;
    hipStream_t s = ctx->stream;
    ev.d_info.reserve(64);
    MC_HIP(hipMemsetAsync(ev.d_info.ptr, 0, 64, s));
    int info[2] = {0, 0};
    {
        TimedScope ts(ctx->timer, s, "ev_scan");
        hipLaunchKernelGGL(mc::k_ev_validate, grid_for(std::max<int64_t>(std::max(in.P, in.npts), in.K + 1)), dim3(256), 0, s,
                           in.P, in.gt, in.K, in.off, in.npts, in.pts, ev.no_class ? 1 : 0, ev.class_ids[0] * 1000,
                           ev.d_info.as<int>());
        MC_HIP(hipGetLastError());
    }
    fetch(ctx, info, ev.d_info.ptr, 8);
    MC_REQUIRE(!(info[0] & 1), MC_ERR_INVALID, "negative ground-truth id");
    MC_REQUIRE(!(info[0] & 4), MC_ERR_INVALID, "prediction offsets must start at 0, ascend and end at num_pred_pts");
    MC_REQUIRE(!(info[0] & 2), MC_ERR_INVALID, "prediction point id out of range");
    return info[1] + 1;
}

// the scan's device arrays, sized by their bounds (R ids, P points, K predictions, npts pairs)
EvScanScratch ev_scan_carve(EvState &ev, const EvScanIn &in, int R)
{
    const int C = ev.C, K = in.K;
    const size_t gcap = static_cast<size_t>(std::min<int64_t>(R, in.P)) + 1;
    ev.d_cnt.reserve(static_cast<size_t>(R) * 4);
    ev.d_inst.reserve(static_cast<size_t>(R) * 4);
    ev.d_tmp_id.reserve(gcap * 4);
    ev.d_class.reserve((3 * static_cast<size_t>(C) + 1) * 4);
    ev.d_gcls.reserve(gcap * 4);
    ev.d_gid.reserve(gcap * 4);
    ev.d_gvert.reserve(gcap * 8);
    ev.d_pinst.reserve(static_cast<size_t>(in.P) * 4 + 8);
    const size_t k8 = (static_cast<size_t>(K) * 4 + 7) & ~size_t(7);
    ev.d_pk.reserve(5 * k8 + 2 * static_cast<size_t>(K) * 8 + 8);
    ev.d_pair_gt.reserve(static_cast<size_t>(in.npts) * 4 + 8);
    ev.d_pair_int.reserve(static_cast<size_t>(in.npts) * 8 + 8);
    // the compact tables as one run of words
    ev.d_out.reserve((3 * gcap + 4 * static_cast<size_t>(K) + 3 * static_cast<size_t>(in.npts) + 1) * 8);
    char *pk = ev.d_pk.as<char>();
    EvScanScratch t;
    t.keep = reinterpret_cast<int *>(pk), t.pcls = reinterpret_cast<int *>(pk + k8);
    t.npair = reinterpret_cast<int *>(pk + 2 * k8), t.kept = reinterpret_cast<int *>(pk + 3 * k8);
    t.pbase = reinterpret_cast<int *>(pk + 4 * k8);
    t.pvert = reinterpret_cast<int64_t *>(pk + 5 * k8), t.pvoid = t.pvert + K;
    t.class_cnt = ev.d_class.as<int>(), t.class_first = t.class_cnt + C, t.class_off = t.class_first + C;
    return t;
}

// instances, kept predictions and their pairs into d_out, the three sizes into d_info + 4 (launches only)
void ev_scan_launch(mc_ctx *ctx, const EvScanIn &in, int R, const EvScanScratch &t)
{
    EvState &ev = ctx->ev;
    hipStream_t s = ctx->stream;
    const int C = ev.C, K = in.K, nc = ev.no_class ? 1 : 0, base = ev.class_ids[0] * 1000;
    const int64_t P = in.P;
    int *sizes = ev.d_info.as<int>() + 4;
    MC_HIP(hipMemsetAsync(ev.d_cnt.ptr, 0, static_cast<size_t>(R) * 4, s));
    MC_HIP(hipMemsetAsync(ev.d_inst.ptr, 0xff, static_cast<size_t>(R) * 4, s));
    MC_HIP(hipMemsetAsync(t.class_cnt, 0, static_cast<size_t>(C) * 4, s));
    MC_HIP(hipMemsetAsync(t.class_first, 0x7f, static_cast<size_t>(C) * 4, s));
    TimedScope ts(ctx->timer, s, "ev_scan");
    if (P && R <= mc::kEvCountLds)
        hipLaunchKernelGGL(mc::k_ev_gt_count_lds, grid_for(P, 2048, 256), dim3(256), 0, s, P, in.gt, nc, base, R,
                           ev.d_cnt.as<int>());
    else if (P)
        hipLaunchKernelGGL(mc::k_ev_gt_count, grid_for(P), dim3(256), 0, s, P, in.gt, nc, base, ev.d_cnt.as<int>());
    hipLaunchKernelGGL(mc::k_ev_gt_table, dim3(1), dim3(1024), 0, s, R, ev.d_cnt.as<int>(), ev.d_lab2cls.as<int>(), ev.nlab, C,
                       ev.d_tmp_id.as<int>(), t.class_cnt, t.class_first, t.class_off, ev.d_gcls.as<int>(), ev.d_gid.as<int>(),
                       ev.d_gvert.as<int64_t>(), ev.d_inst.as<int>(), sizes);
    if (P)
        hipLaunchKernelGGL(mc::k_ev_point_inst, grid_for(P), dim3(256), 0, s, P, in.gt, nc, base, ev.d_lab2cls.as<int>(),
                           ev.nlab, ev.d_inst.as<int>(), ev.d_pinst.as<int>());
    if (K)
        hipLaunchKernelGGL(mc::k_ev_inter, dim3(std::min(K, 8192)), dim3(256), 0, s, K, in.off, in.pts, in.pcls, nc,
                           ev.d_lab2cls.as<int>(), ev.nlab, static_cast<int>(std::min<int64_t>(ev.min_region, INT32_MAX)),
                           ev.d_pinst.as<int>(), t.class_off, t.keep, t.pcls, t.pvert, t.pvoid, t.npair,
                           ev.d_pair_gt.as<int>(), ev.d_pair_int.as<int64_t>());
    hipLaunchKernelGGL(mc::k_ev_pred_scan, dim3(1), dim3(1024), 0, s, K, t.keep, t.npair, t.kept, t.pbase, sizes);
    hipLaunchKernelGGL(mc::k_ev_compact, dim3(std::max(1, std::min(K, 8192))), dim3(256), 0, s, K, in.off, t.keep, t.kept,
                       t.pbase, t.npair, t.pcls, t.pvert, t.pvoid, in.pscore, ev.d_pair_gt.as<int>(),
                       ev.d_pair_int.as<int64_t>(), ev.d_gcls.as<int>(), ev.d_gid.as<int>(), ev.d_gvert.as<int64_t>(), sizes,
                       ev.d_out.as<int64_t>());
    MC_HIP(hipGetLastError());
}

// the sizes, then the compact tables, to the host
EvTables ev_scan_fetch(mc_ctx *ctx)
{
    EvState &ev = ctx->ev;
    int n[3] = {0, 0, 0};  // instances, kept predictions, pairs
    fetch(ctx, n, ev.d_info.as<int>() + 4, 12);
    const size_t words = mc::ev_compact_words(n[0], n[1], n[2]);
    ev.h_out.resize(words + 1);
    fetch(ctx, ev.h_out.data(), ev.d_out.ptr, words * 8);
    ctx->timer.collect();
    return mc::ev_unpack_tables(ev.h_out.data(), n[0], n[1], n[2]);
}

void ev_scan_device(mc_ctx *ctx, const EvScanIn &in)
{
    const int R = ev_scan_validate(ctx, in);
    const EvScanScratch t = ev_scan_carve(ctx->ev, in, R);
    ev_scan_launch(ctx, in, R, t);
    ev_commit(ctx, ev_scan_fetch(ctx));
}

// every unit's examples into its cell's segment of d_key / d_true (launches only); returns cell_off [NC + 1]
int *ev_segments(mc_ctx *ctx)
{
    EvState &ev = ctx->ev;
    hipStream_t s = ctx->stream;
    const int NC = ev.C * ev.O, U = ev.units;
    const size_t n = static_cast<size_t>(ev.ex_used);
    ev.d_key.reserve(n * 8 + 8);
    ev.d_true.reserve(n + 8);
    ev.d_cell.reserve((3 * static_cast<size_t>(NC) + 1) * 4);
    int *cell_n = ev.d_cell.as<int>(), *cell_fill = cell_n + NC, *cell_off = cell_fill + NC;
    MC_HIP(hipMemsetAsync(cell_n, 0, 2 * static_cast<size_t>(NC) * 4, s));
    if (U)
        hipLaunchKernelGGL(mc::k_ev_cell_count, grid_for(U), dim3(256), 0, s, U, ev.d_unit_cell.as<int>(),
                           ev.d_unit_cnt.as<int>(), cell_n);
    hipLaunchKernelGGL(mc::k_ev_cell_scan, dim3(1), dim3(1024), 0, s, NC, cell_n, cell_off);
    if (U)
        hipLaunchKernelGGL(mc::k_ev_gather, dim3(std::min(U, 8192)), dim3(256), 0, s, U, ev.d_unit_cell.as<int>(),
                           ev.d_unit_cnt.as<int>(), ev.d_unit_off.as<int64_t>(), cell_off, cell_fill,
                           ev.d_ex_key.as<unsigned long long>(), ev.d_ex_true.as<unsigned char>(),
                           ev.d_key.as<unsigned long long>(), ev.d_true.as<unsigned char>());
    return cell_off;
}

// the table over everything accumulated; curve_cell >= 0 also fills that cell's curve (device arrays)
void ev_compute(mc_ctx *ctx, int curve_cell, double *cv_score, int64_t *cv_tp, int64_t *cv_fp, int64_t *cv_fn)
{
    EvState &ev = ctx->ev;
    hipStream_t s = ctx->stream;
    const int NC = ev.C * ev.O;
    const size_t n = static_cast<size_t>(ev.ex_used);
    ev.d_prec.reserve((n + NC) * 8 + 8);
    ev.d_rec.reserve((n + NC) * 8 + 8);
    ev.d_ap.reserve(static_cast<size_t>(NC) * 8);
    ev.d_stats.reserve(static_cast<size_t>(NC) * 32);
    ev.d_ndist.reserve(static_cast<size_t>(NC) * 4);
    {
        TimedScope ts(ctx->timer, s, "ev_ap");
        const int *cell_off = ev_segments(ctx);
        hipLaunchKernelGGL(mc::k_ev_ap, dim3(std::min(NC, 8192)), dim3(256), 0, s, NC, cell_off,
                           ev.d_key.as<unsigned long long>(), ev.d_true.as<unsigned char>(),
                           ev.d_hardfn.as<unsigned long long>(), ev.d_flags.as<unsigned>(), ev.d_prec.as<double>(),
                           ev.d_rec.as<double>(), ev.d_ap.as<double>(), ev.d_stats.as<int64_t>(), ev.d_ndist.as<int>(),
                           curve_cell, cv_score, cv_tp, cv_fp, cv_fn);
        MC_HIP(hipGetLastError());
    }
    ev.ap.resize(NC), ev.stats.resize(static_cast<size_t>(NC) * 4), ev.ndist.resize(NC);
    MC_HIP(hipMemcpyAsync(ev.ap.data(), ev.d_ap.ptr, static_cast<size_t>(NC) * 8, hipMemcpyDeviceToHost, s));
    MC_HIP(hipMemcpyAsync(ev.stats.data(), ev.d_stats.ptr, static_cast<size_t>(NC) * 32, hipMemcpyDeviceToHost, s));
    MC_HIP(hipMemcpyAsync(ev.ndist.data(), ev.d_ndist.ptr, static_cast<size_t>(NC) * 4, hipMemcpyDeviceToHost, s));
    MC_HIP(hipStreamSynchronize(s));
    ctx->timer.collect();
    ev.ap_valid = true;
}

// ---- the accumulation as a state buffer (include/mcgraph.h, mc_ev_state_*) -----------------------

// the state buffer of the accumulation in d_state, kept until the accumulation changes
void ev_runs(mc_ctx *ctx)
{
    EvState &ev = ctx->ev;
    if (ev.runs_valid) return;
    hipStream_t s = ctx->stream;
    const int C = ev.C, O = ev.O, NC = C * O;
    ev.d_run.reserve((2 * static_cast<size_t>(NC) + 1) * 4);
    int *cell_nrun = ev.d_run.as<int>(), *run_off = cell_nrun + NC;
    int *cell_off;
    {
        TimedScope ts(ctx->timer, s, "ev_state");
        cell_off = ev_segments(ctx);
        hipLaunchKernelGGL(mc::k_ev_run_count, dim3(std::min(NC, 8192)), dim3(256), 0, s, NC, cell_off,
                           ev.d_key.as<unsigned long long>(), ev.d_true.as<unsigned char>(), cell_nrun);
        hipLaunchKernelGGL(mc::k_ev_cell_scan, dim3(1), dim3(1024), 0, s, NC, cell_nrun, run_off);
        MC_HIP(hipGetLastError());
    }
    int tot[2] = {0, 0};  // runs, examples
    MC_HIP(hipMemcpyAsync(&tot[0], run_off + NC, 4, hipMemcpyDeviceToHost, s));
    MC_HIP(hipMemcpyAsync(&tot[1], cell_off + NC, 4, hipMemcpyDeviceToHost, s));
    MC_HIP(hipStreamSynchronize(s));
    const int64_t R = tot[0];
    const mc::EvLayout L = mc::ev_layout(C, O, R);
    std::vector<int64_t> head(L.roff / 8, 0);
    head[0] = mc::kEvStateWord, head[1] = C, head[2] = O, head[3] = ev.min_region, head[4] = ev.no_class ? 1 : 0, head[5] = R;
    char *hb = reinterpret_cast<char *>(head.data());
    std::memcpy(hb + L.ids, ev.class_ids.data(), static_cast<size_t>(C) * 4);
    std::memcpy(hb + L.ov, ev.overlaps.data(), static_cast<size_t>(O) * 8);
    ev.d_state.reserve(L.bytes);
    char *D = ev.d_state.as<char>();
    MC_HIP(hipMemsetAsync(D, 0, L.bytes, s));  // the padding of the 4-byte sections
    MC_HIP(hipMemcpyAsync(D, hb, L.roff, hipMemcpyHostToDevice, s));
    {
        TimedScope ts(ctx->timer, s, "ev_state");
        hipLaunchKernelGGL(mc::k_ev_run_write, dim3(std::min(NC, 8192)), dim3(256), 0, s, NC, cell_off,
                           ev.d_key.as<unsigned long long>(), ev.d_true.as<unsigned char>(), run_off,
                           ev.d_hardfn.as<unsigned long long>(), ev.d_flags.as<unsigned>(),
                           reinterpret_cast<int64_t *>(D + L.roff), reinterpret_cast<int64_t *>(D + L.hf),
                           reinterpret_cast<unsigned *>(D + L.fl), reinterpret_cast<unsigned long long *>(D + L.key),
                           reinterpret_cast<unsigned *>(D + L.nt), reinterpret_cast<unsigned *>(D + L.nf));
        MC_HIP(hipGetLastError());
    }
    MC_HIP(hipStreamSynchronize(s));  // the upload reads this call's host words
    ctx->timer.collect();
    ev.state_runs = R, ev.state_examples = tot[1], ev.state_bytes = static_cast<int64_t>(L.bytes);
    ev.runs_valid = true;
}

// ---- mc_ev_state_merge ---------------------------------------------------------------------------
struct EvMergeSrc {
    const char *buf;
    int64_t bytes;
    bool on_device;
};

// The header, then (once it is known to fit) the sections up to the keys, to the host and through the checks
// of mc_ap_plan.hpp: two fetches for a device buffer.  Returns the layout; cells: the cells with runs.
mc::EvLayout ev_merge_parse(mc_ctx *ctx, const EvMergeSrc &m, std::vector<int> &cells)
{
    const EvState &ev = ctx->ev;
    auto take = [&](void *dst, size_t at, size_t n) {  // a part of the buffer to the host
        if (m.on_device) fetch(ctx, dst, m.buf + at, n);
        else std::memcpy(dst, m.buf + at, n);
    };
    const bool has_header = m.buf && m.bytes >= static_cast<int64_t>(mc::kEvStateHeader);
    MC_REQUIRE(!has_header || !m.on_device || (reinterpret_cast<uintptr_t>(m.buf) & 7) == 0, MC_ERR_INVALID,
               "state buffer must be 8-byte aligned");
    int64_t hdr[6], R = 0;
    if (has_header) take(hdr, 0, mc::kEvStateHeader);
    ev_require(mc::ev_check_state_header(has_header ? hdr : nullptr, m.bytes, ev.C, ev.O, ev.min_region, ev.no_class, R),
               MC_ERR_INVALID);
    const mc::EvLayout L = mc::ev_layout(ev.C, ev.O, R);
    std::vector<int64_t> mid((L.key - L.ids) / 8);
    take(mid.data(), L.ids, L.key - L.ids);
    ev_require(mc::ev_check_state_sections(mid.data(), L, ev.class_ids, ev.overlaps, cells), MC_ERR_INVALID);
    return L;
}

// the buffer's sections on the device (a host buffer is uploaded to d_merge)
struct EvStateDev {
    const int64_t *roff, *hf;
    const unsigned *fl, *nt, *nf;
    const unsigned long long *key;
};

EvStateDev ev_merge_sections(mc_ctx *ctx, const EvMergeSrc &m, const mc::EvLayout &L)
{
    EvState &ev = ctx->ev;
    const char *D = m.buf;
    if (!m.on_device) {
        ev.d_merge.reserve(L.bytes);
        MC_HIP(hipMemcpyAsync(ev.d_merge.ptr, m.buf, L.bytes, hipMemcpyHostToDevice, ctx->stream));
        D = ev.d_merge.as<char>();
    }
    EvStateDev d;
    d.roff = reinterpret_cast<const int64_t *>(D + L.roff), d.hf = reinterpret_cast<const int64_t *>(D + L.hf);
    d.fl = reinterpret_cast<const unsigned *>(D + L.fl);
    d.key = reinterpret_cast<const unsigned long long *>(D + L.key);
    d.nt = reinterpret_cast<const unsigned *>(D + L.nt), d.nf = reinterpret_cast<const unsigned *>(D + L.nf);
    return d;
}

// the run checks behind one flag word; returns the examples of all runs
unsigned long long ev_merge_check_runs(mc_ctx *ctx, const EvStateDev &d, int64_t R)
{
    EvState &ev = ctx->ev;
    hipStream_t s = ctx->stream;
    ev.d_info.reserve(64);
    MC_HIP(hipMemsetAsync(ev.d_info.ptr, 0, 16, s));
    if (R) {
        TimedScope ts(ctx->timer, s, "ev_merge");
        hipLaunchKernelGGL(mc::k_ev_state_check, grid_for(R), dim3(256), 0, s, ev.C * ev.O, R, d.roff, d.key, d.nt, d.nf,
                           ev.d_info.as<int>(), reinterpret_cast<unsigned long long *>(ev.d_info.as<char>() + 8));
        MC_HIP(hipGetLastError());
    }
    unsigned long long chk[2] = {0, 0};
    fetch(ctx, chk, ev.d_info.ptr, 16);
    const int bad = static_cast<int>(chk[0] & 0xffffffffu);
    MC_REQUIRE(!(bad & 1), MC_ERR_INVALID, "a run without examples");
    MC_REQUIRE(!(bad & 2), MC_ERR_INVALID, "a key that is no score (NaN)");
    MC_REQUIRE(!(bad & 4), MC_ERR_INVALID, "keys must ascend strictly within a cell");
    return chk[1];
}

// the runs' examples behind the accumulation's, one unit per cell with runs (launches only)
void ev_merge_expand(mc_ctx *ctx, const EvStateDev &d, int64_t R, int64_t add, const std::vector<int> &cells)
{
    EvState &ev = ctx->ev;
    hipStream_t s = ctx->stream;
    const int NC = ev.C * ev.O, U = static_cast<int>(cells.size());
    ev.d_tmp.reserve(static_cast<size_t>(U) * 4 + 8);
    ev.d_words.reserve((static_cast<size_t>(R) + 1) * 4 + 8);
    if (U) MC_HIP(hipMemcpyAsync(ev.d_tmp.ptr, cells.data(), static_cast<size_t>(U) * 4, hipMemcpyHostToDevice, s));
    int *run_ex = ev.d_words.as<int>();
    TimedScope ts(ctx->timer, s, "ev_merge");
    if (R) {
        hipLaunchKernelGGL(mc::k_ev_state_scan, dim3(1), dim3(1024), 0, s, static_cast<int>(R), d.nt, d.nf, run_ex);
        hipLaunchKernelGGL(mc::k_ev_state_expand, grid_for(add), dim3(256), 0, s, static_cast<int>(R), run_ex, d.key, d.nt,
                           ev.d_ex_key.as<unsigned long long>() + ev.ex_used, ev.d_ex_true.as<unsigned char>() + ev.ex_used);
    }
    hipLaunchKernelGGL(mc::k_ev_state_units, grid_for(std::max(NC, U)), dim3(256), 0, s, NC, U, ev.d_tmp.as<int>(), d.roff,
                       run_ex, d.hf, d.fl, ev.ex_used, ev.d_unit_cell.as<int>() + ev.units, ev.d_unit_cnt.as<int>() + ev.units,
                       ev.d_unit_off.as<int64_t>() + ev.units, ev.d_hardfn.as<unsigned long long>(), ev.d_flags.as<unsigned>());
    MC_HIP(hipGetLastError());
}

void ev_merge(mc_ctx *ctx, const EvMergeSrc &m)
{
    EvState &ev = ctx->ev;
    hipStream_t s = ctx->stream;
    std::vector<int> cells;
    const mc::EvLayout L = ev_merge_parse(ctx, m, cells);
    const int64_t R = static_cast<int64_t>((L.nt - L.key) / 8);
    const int U = static_cast<int>(cells.size());
    const EvStateDev d = ev_merge_sections(ctx, m, L);
    const unsigned long long total = ev_merge_check_runs(ctx, d, R);
    ev_require(mc::ev_check_append(ev.ex_used, ev.units, total, U), MC_ERR_UNSUPPORTED);
    // ---- from here on the accumulation changes ----
    const int64_t add = static_cast<int64_t>(total);
    ev_reserve_append(ev, add, U, s);
    ev_merge_expand(ctx, d, R, add, cells);
    MC_HIP(hipStreamSynchronize(s));  // the uploads read this call's host words
    ctx->timer.collect();
    ev.ex_used += add;
    ev.units += U;
    ev.ap_valid = false;
    ev.runs_valid = false;
}

}  // namespace

extern "C" {

int mc_ev_begin(mc_ctx *ctx, int32_t num_classes, const int32_t *class_ids, int32_t num_overlaps, const double *overlaps,
                int64_t min_region_size, int no_class)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(num_classes >= 1 && class_ids && overlaps, MC_ERR_INVALID, "null or empty class table");
        MC_REQUIRE(num_overlaps >= 1 && num_overlaps <= mc::kEvMaxOverlaps, MC_ERR_INVALID, "1 to 32 overlaps");
        MC_REQUIRE(min_region_size >= 0, MC_ERR_INVALID, "negative min_region_size");
        int mx = 0;
        for (int c = 0; c < num_classes; c++) {
            MC_REQUIRE(class_ids[c] >= 0 && class_ids[c] < 2000000, MC_ERR_INVALID, "class id out of range");
            mx = std::max(mx, class_ids[c]);
        }
        for (int o = 0; o < num_overlaps; o++) MC_REQUIRE(!std::isnan(overlaps[o]), MC_ERR_INVALID, "overlap is NaN");
        std::vector<int32_t> lab2cls(static_cast<size_t>(mx) + 1, -1);
        for (int c = 0; c < num_classes; c++) {
            MC_REQUIRE(lab2cls[class_ids[c]] < 0, MC_ERR_INVALID, "class id twice");
            lab2cls[class_ids[c]] = c;
        }
        EvState &ev = ctx->ev;
        hipStream_t s = ctx->stream;
        const size_t NC = static_cast<size_t>(num_classes) * num_overlaps;
        ev.d_lab2cls.reserve(lab2cls.size() * 4);
        ev.d_overlaps.reserve(static_cast<size_t>(num_overlaps) * 8);
        ev.d_hardfn.reserve(NC * 8);
        ev.d_flags.reserve(NC * 4);
        MC_HIP(hipMemcpyAsync(ev.d_lab2cls.ptr, lab2cls.data(), lab2cls.size() * 4, hipMemcpyHostToDevice, s));
        MC_HIP(hipMemcpyAsync(ev.d_overlaps.ptr, overlaps, static_cast<size_t>(num_overlaps) * 8, hipMemcpyHostToDevice, s));
        MC_HIP(hipMemsetAsync(ev.d_hardfn.ptr, 0, NC * 8, s));
        MC_HIP(hipMemsetAsync(ev.d_flags.ptr, 0, NC * 4, s));
        MC_HIP(hipStreamSynchronize(s));
        ev.C = num_classes, ev.O = num_overlaps, ev.nlab = mx + 1;
        ev.class_ids.assign(class_ids, class_ids + num_classes);
        ev.overlaps.assign(overlaps, overlaps + num_overlaps);
        ev.min_region = min_region_size;
        ev.no_class = no_class != 0;
        ev.ex_used = 0, ev.units = 0;
        ev.have_last = false, ev.ap_valid = false, ev.runs_valid = false;
        ev.active = true;
    });
}

int mc_ev_add_scan(mc_ctx *ctx, int64_t num_points, const int32_t *gt_ids, int32_t num_pred, const int64_t *pred_off,
                   int64_t num_pred_pts, const int32_t *pred_pts, const int32_t *pred_classes, const double *pred_scores,
                   int on_device)
{
    return guarded(ctx, [&] {
        EvState &ev = ctx->ev;
        MC_REQUIRE(ev.active, MC_ERR_STATE, "mc_ev_begin first");
        MC_REQUIRE(num_points >= 0 && num_points < INT32_MAX && num_pred >= 0 && num_pred_pts >= 0 && num_pred_pts < INT32_MAX,
                   MC_ERR_INVALID, "bad size");
        MC_REQUIRE(pred_off && (num_points == 0 || gt_ids) && (num_pred_pts == 0 || pred_pts), MC_ERR_INVALID, "null argument");
        if (on_device) {
            ev_scan_device(ctx, {num_points, gt_ids, num_pred, pred_off, num_pred_pts, pred_pts, pred_classes, pred_scores});
            return;
        }
        hipStream_t s = ctx->stream;
        const void *src[5] = {gt_ids, pred_off, pred_pts, pred_classes, pred_scores};
        const size_t bytes[5] = {static_cast<size_t>(num_points) * 4, (static_cast<size_t>(num_pred) + 1) * 8,
                                 static_cast<size_t>(num_pred_pts) * 4, static_cast<size_t>(num_pred) * 4,
                                 static_cast<size_t>(num_pred) * 8};
        for (int i = 0; i < 5; i++) {
            ev.d_in[i].reserve(bytes[i] + 8);
            if (src[i] && bytes[i]) MC_HIP(hipMemcpyAsync(ev.d_in[i].ptr, src[i], bytes[i], hipMemcpyHostToDevice, s));
        }
        ev_scan_device(ctx, {num_points, ev.d_in[0].as<int>(), num_pred, ev.d_in[1].as<int64_t>(), num_pred_pts,
                             ev.d_in[2].as<int>(), pred_classes ? ev.d_in[3].as<int>() : nullptr,
                             pred_scores ? ev.d_in[4].as<double>() : nullptr});
    });
}

int mc_ev_add_scan_clustered(mc_ctx *ctx, const int32_t *gt_ids, int on_device)
{
    return guarded(ctx, [&] {
        PpState &pp = ctx->pp;
        EvState &ev = ctx->ev;
        MC_REQUIRE(ev.active, MC_ERR_STATE, "mc_ev_begin first");
        MC_REQUIRE(pp.have, MC_ERR_STATE, "no post-processing result");
        pp_build_export(ctx);
        const int nf = pp.info.num_final;
        const int64_t P = pp.P, np = pp.opoff[nf];
        MC_REQUIRE(P == 0 || gt_ids, MC_ERR_INVALID, "null argument");
        MC_REQUIRE(P < INT32_MAX && np < INT32_MAX, MC_ERR_UNSUPPORTED, "scene too large");
        const int *gt = gt_ids;
        if (!on_device) {
            ev.d_in[0].reserve(static_cast<size_t>(P) * 4 + 8);
            if (P) MC_HIP(hipMemcpyAsync(ev.d_in[0].ptr, gt_ids, static_cast<size_t>(P) * 4, hipMemcpyHostToDevice, ctx->stream));
            gt = ev.d_in[0].as<int>();
        }
        ev_scan_device(ctx, {P, gt, nf, pp.d_opoff.as<int64_t>(), np, pp.d_opts.as<int>(), nullptr, nullptr});
    });
}

int mc_ev_add_matches(mc_ctx *ctx, int32_t num_gt, const int32_t *gt_class, const int32_t *gt_id, const int64_t *gt_vert,
                      int32_t num_pred, const int32_t *pred_class, const int64_t *pred_vert, const int64_t *pred_void,
                      const double *pred_score, int64_t num_pairs, const int32_t *pair_pred, const int32_t *pair_gt,
                      const int64_t *pair_int)
{
    return guarded(ctx, [&] {
        EvState &ev = ctx->ev;
        MC_REQUIRE(ev.active, MC_ERR_STATE, "mc_ev_begin first");
        MC_REQUIRE(num_gt >= 0 && num_pred >= 0 && num_pairs >= 0 && num_pairs < INT32_MAX, MC_ERR_INVALID, "bad size");
        MC_REQUIRE((num_gt == 0 || (gt_class && gt_id && gt_vert)) &&
                       (num_pred == 0 || (pred_class && pred_vert && pred_void && pred_score)) &&
                       (num_pairs == 0 || (pair_pred && pair_gt && pair_int)),
                   MC_ERR_INVALID, "null argument");
        EvTables t;
        t.gcls.assign(gt_class, gt_class + num_gt), t.gid.assign(gt_id, gt_id + num_gt), t.gvert.assign(gt_vert, gt_vert + num_gt);
        t.pcls.assign(pred_class, pred_class + num_pred), t.pvert.assign(pred_vert, pred_vert + num_pred);
        t.pvoid.assign(pred_void, pred_void + num_pred), t.pscore.assign(pred_score, pred_score + num_pred);
        t.ppred.assign(pair_pred, pair_pred + num_pairs), t.pgt.assign(pair_gt, pair_gt + num_pairs);
        t.pint.assign(pair_int, pair_int + num_pairs);
        ev_commit(ctx, std::move(t));
    });
}

int mc_ev_scan_info(mc_ctx *ctx, int32_t *num_gt, int32_t *num_pred, int64_t *num_pairs)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->ev.active && ctx->ev.have_last, MC_ERR_STATE, "no scan added");
        if (num_gt) *num_gt = static_cast<int32_t>(ctx->ev.last.gcls.size());
        if (num_pred) *num_pred = static_cast<int32_t>(ctx->ev.last.pcls.size());
        if (num_pairs) *num_pairs = static_cast<int64_t>(ctx->ev.last.ppred.size());
    });
}

int mc_ev_get_scan(mc_ctx *ctx, int32_t *gt_class, int32_t *gt_id, int64_t *gt_vert, int32_t *pred_class,
                   int64_t *pred_vert, int64_t *pred_void, double *pred_score, int32_t *pair_pred, int32_t *pair_gt,
                   int64_t *pair_int)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->ev.active && ctx->ev.have_last, MC_ERR_STATE, "no scan added");
        const EvTables &t = ctx->ev.last;
        auto cp = [](void *dst, const void *src, size_t bytes) {
            if (dst && bytes) std::memcpy(dst, src, bytes);
        };
        cp(gt_class, t.gcls.data(), t.gcls.size() * 4), cp(gt_id, t.gid.data(), t.gid.size() * 4);
        cp(gt_vert, t.gvert.data(), t.gvert.size() * 8), cp(pred_class, t.pcls.data(), t.pcls.size() * 4);
        cp(pred_vert, t.pvert.data(), t.pvert.size() * 8), cp(pred_void, t.pvoid.data(), t.pvoid.size() * 8);
        cp(pred_score, t.pscore.data(), t.pscore.size() * 8), cp(pair_pred, t.ppred.data(), t.ppred.size() * 4);
        cp(pair_gt, t.pgt.data(), t.pgt.size() * 4), cp(pair_int, t.pint.data(), t.pint.size() * 8);
    });
}

int mc_ev_ap(mc_ctx *ctx, double *ap, int64_t *stats)
{
    return guarded(ctx, [&] {
        EvState &ev = ctx->ev;
        MC_REQUIRE(ev.active, MC_ERR_STATE, "mc_ev_begin first");
        if (!ev.ap_valid) ev_compute(ctx, -1, nullptr, nullptr, nullptr, nullptr);
        if (ap) std::memcpy(ap, ev.ap.data(), ev.ap.size() * 8);
        if (stats) std::memcpy(stats, ev.stats.data(), ev.stats.size() * 8);
    });
}

int mc_ev_get_curve(mc_ctx *ctx, int32_t class_index, int32_t overlap_index, int64_t *num_scores, double *scores,
                    int64_t *tp, int64_t *fp, int64_t *fn)
{
    return guarded(ctx, [&] {
        EvState &ev = ctx->ev;
        MC_REQUIRE(ev.active, MC_ERR_STATE, "mc_ev_begin first");
        MC_REQUIRE(class_index >= 0 && class_index < ev.C && overlap_index >= 0 && overlap_index < ev.O, MC_ERR_INVALID,
                   "cell out of range");
        if (!ev.ap_valid) ev_compute(ctx, -1, nullptr, nullptr, nullptr, nullptr);
        const int cell = class_index * ev.O + overlap_index;
        const int64_t n = ev.stats[4 * static_cast<size_t>(cell) + 3] == 3 ? ev.ndist[cell] : 0;
        if (num_scores) *num_scores = n;
        if (!n || !(scores || tp || fp || fn)) return;
        DevBuf cv;
        cv.reserve(static_cast<size_t>(n) * 32);
        double *d_score = cv.as<double>();
        int64_t *d_tp = reinterpret_cast<int64_t *>(d_score + n), *d_fp = d_tp + n, *d_fn = d_fp + n;
        ev_compute(ctx, cell, d_score, d_tp, d_fp, d_fn);
        hipStream_t s = ctx->stream;
        auto dn = [&](void *dst, const void *src) {
            if (dst) MC_HIP(hipMemcpyAsync(dst, src, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost, s));
        };
        dn(scores, d_score), dn(tp, d_tp), dn(fp, d_fp), dn(fn, d_fn);
        MC_HIP(hipStreamSynchronize(s));
    });
}

int mc_ev_state_info(mc_ctx *ctx, int64_t *num_runs, int64_t *num_examples, int64_t *bytes)
{
    return guarded(ctx, [&] {
        EvState &ev = ctx->ev;
        MC_REQUIRE(ev.active, MC_ERR_STATE, "mc_ev_begin first");
        ev_runs(ctx);
        if (num_runs) *num_runs = ev.state_runs;
        if (num_examples) *num_examples = ev.state_examples;
        if (bytes) *bytes = ev.state_bytes;
    });
}

int mc_ev_state_export(mc_ctx *ctx, void *buf, int64_t bytes, int on_device)
{
    return guarded(ctx, [&] {
        EvState &ev = ctx->ev;
        MC_REQUIRE(ev.active, MC_ERR_STATE, "mc_ev_begin first");
        ev_runs(ctx);
        MC_REQUIRE(buf && bytes >= ev.state_bytes, MC_ERR_INVALID, "buffer smaller than mc_ev_state_info reports");
        hipStream_t s = ctx->stream;
        MC_HIP(hipMemcpyAsync(buf, ev.d_state.ptr, static_cast<size_t>(ev.state_bytes),
                              on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        MC_HIP(hipStreamSynchronize(s));
    });
}

int mc_ev_state_merge(mc_ctx *ctx, const void *buf, int64_t bytes, int on_device)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->ev.active, MC_ERR_STATE, "mc_ev_begin first");
        ev_merge(ctx, {static_cast<const char *>(buf), bytes, on_device != 0});
    });
}

}  // extern "C"
