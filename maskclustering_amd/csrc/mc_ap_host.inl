// mc_ap_host.inl — host side of the AP evaluation (mc_ev_*, include/mcgraph.h); kernels in
// mc_ap_kernels.inl.  Included by mc_api.hip after the post-processing section.
//
// A scan reaches the accumulation in two halves.  mc_ev_add_scan* turn ground-truth ids and point
// lists into the scan's compact tables on the device (instances, kept predictions, non-zero
// same-class intersections) and fetch them: O(instances + predictions + pairs) words.  commit()
// (shared with mc_ev_add_matches) lays the tables out per class, uploads them and runs the greedy
// pass, which appends (score, true) examples to per-(scan, class, overlap) regions whose sizes
// are known beforehand.  All checks come before the first write to the accumulation.
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

void ev_commit(mc_ctx *ctx, EvTables &&t)
{
    EvState &ev = ctx->ev;
    hipStream_t s = ctx->stream;
    const int G = static_cast<int>(t.gcls.size()), K = static_cast<int>(t.pcls.size()), C = ev.C, O = ev.O;
    const int64_t NP = static_cast<int64_t>(t.ppred.size());
    for (int g = 0; g < G; g++) {
        MC_REQUIRE(t.gcls[g] >= 0 && t.gcls[g] < C && (g == 0 || t.gcls[g] >= t.gcls[g - 1]), MC_ERR_INVALID,
                   "ground-truth classes must be ascending class indices");
        MC_REQUIRE(t.gvert[g] > 0, MC_ERR_INVALID, "ground-truth vert_count must be positive");
    }
    for (int k = 0; k < K; k++) {
        MC_REQUIRE(t.pcls[k] >= 0 && t.pcls[k] < C, MC_ERR_INVALID, "prediction class index out of range");
        MC_REQUIRE(t.pvert[k] > 0 && t.pvoid[k] >= 0 && t.pvoid[k] <= t.pvert[k], MC_ERR_INVALID, "bad prediction counts");
        MC_REQUIRE(!std::isnan(t.pscore[k]), MC_ERR_INVALID, "prediction score is NaN");
    }
    std::vector<int64_t> gt_poff(static_cast<size_t>(G) + 1, 0);
    for (int64_t i = 0; i < NP; i++) {
        const int p = t.ppred[i], g = t.pgt[i];
        MC_REQUIRE(p >= 0 && p < K && g >= 0 && g < G, MC_ERR_INVALID, "pair index out of range");
        MC_REQUIRE(t.gcls[g] == t.pcls[p], MC_ERR_INVALID, "pair across classes");
        MC_REQUIRE(t.pint[i] > 0 && t.pint[i] <= t.gvert[g] && t.pint[i] <= t.pvert[p], MC_ERR_INVALID,
                   "bad intersection");
        gt_poff[g + 1]++;
    }
    for (int g = 0; g < G; g++) gt_poff[g + 1] += gt_poff[g];
    // class slots: the classes with an instance or a prediction in this scan
    std::vector<int> slot(C, -1), g0(C, 0), g1(C, 0), npred(C, 0);
    std::vector<int64_t> nfilt(C, 0);
    for (int g = 0; g < G; g++) {
        const int c = t.gcls[g];
        if (g1[c] == 0 && (g == 0 || t.gcls[g - 1] != c)) g0[c] = g;
        g1[c] = g + 1;
        if (t.gid[g] >= 1000 && t.gvert[g] >= ev.min_region) nfilt[c]++;
    }
    for (int k = 0; k < K; k++) npred[t.pcls[k]]++;
    int A = 0;
    std::vector<int> cls_of;
    for (int c = 0; c < C; c++)
        if (g1[c] > g0[c] || npred[c]) {
            slot[c] = A++;
            cls_of.push_back(c);
        }
    // the words of EvScanDev
    const size_t words = 2 * static_cast<size_t>(G) + 4 * static_cast<size_t>(K) + 3 * static_cast<size_t>(NP) + 7 * static_cast<size_t>(A);
    std::vector<int64_t> W(words + 1, 0);
    int64_t *gvert = W.data(), *gid = gvert + G, *pvert = gid + G, *pvoid = pvert + K, *pslot = pvoid + K;
    double *pscore = reinterpret_cast<double *>(pslot + K);
    int64_t *q_gt = pslot + 2 * K, *q_pred = q_gt + NP, *q_int = q_pred + NP;
    int64_t *s_p0 = q_int + NP, *s_p1 = s_p0 + A, *s_nfilt = s_p1 + A, *s_npred = s_nfilt + A, *s_cls = s_npred + A,
            *s_exoff = s_cls + A, *s_cap = s_exoff + A;
    for (int g = 0; g < G; g++) {
        gvert[g] = t.gvert[g];
        gid[g] = t.gid[g];
    }
    for (int k = 0; k < K; k++) {
        pvert[k] = t.pvert[k];
        pvoid[k] = t.pvoid[k];
        pslot[k] = slot[t.pcls[k]];
        pscore[k] = t.pscore[k];
    }
    {
        std::vector<int64_t> at(gt_poff.begin(), gt_poff.end() - 1);  // stable: a ground truth keeps the list's order
        for (int64_t i = 0; i < NP; i++) {
            const int64_t j = at[t.pgt[i]]++;
            q_gt[j] = t.pgt[i];
            q_pred[j] = t.ppred[i];
            q_int[j] = t.pint[i];
        }
    }
    int64_t total = 0;
    for (int a = 0; a < A; a++) {
        const int c = cls_of[a];
        const bool has = g1[c] > g0[c];
        s_p0[a] = has ? gt_poff[g0[c]] : 0;
        s_p1[a] = has ? gt_poff[g1[c]] : 0;
        s_nfilt[a] = nfilt[c];
        s_npred[a] = npred[c];
        s_cls[a] = c;
        s_cap[a] = (s_p1[a] - s_p0[a]) + npred[c];
        s_exoff[a] = total;
        total += s_cap[a] * O;
    }
    const int U = A * O;
    MC_REQUIRE(ev.ex_used + total < (int64_t(1) << 31) && static_cast<int64_t>(ev.units) + U < (int64_t(1) << 31),
               MC_ERR_UNSUPPORTED, "more than 2^31 examples");
    // ---- from here on the accumulation changes ----
    ev_grow(ev.d_ex_key, ev.ex_used * 8, (ev.ex_used + total) * 8 + 8, s);
    ev_grow(ev.d_ex_true, ev.ex_used, ev.ex_used + total + 8, s);
    ev_grow(ev.d_unit_cell, static_cast<size_t>(ev.units) * 4, static_cast<size_t>(ev.units + U) * 4 + 8, s);
    ev_grow(ev.d_unit_cnt, static_cast<size_t>(ev.units) * 4, static_cast<size_t>(ev.units + U) * 4 + 8, s);
    ev_grow(ev.d_unit_off, static_cast<size_t>(ev.units) * 8, static_cast<size_t>(ev.units + U) * 8 + 8, s);
    if (A) {
        ev.d_words.reserve(words * 8 + 8);
        MC_HIP(hipMemcpyAsync(ev.d_words.ptr, W.data(), words * 8, hipMemcpyHostToDevice, s));
        const size_t b_q = static_cast<size_t>(NP) * 4, b_f = static_cast<size_t>(K) * 4, b_i = static_cast<size_t>(K) * 8,
                     b_v = static_cast<size_t>(O) * K;
        const size_t o_i = 0, o_q = o_i + b_i, o_f = o_q + ((b_q + 7) & ~size_t(7)), o_v = o_f + ((b_f + 7) & ~size_t(7));
        ev.d_tmp.reserve(o_v + b_v + 8);
        MC_HIP(hipMemsetAsync(ev.d_tmp.ptr, 0, o_v + b_v + 8, s));
        const int64_t *D = ev.d_words.as<int64_t>();
        char *T = ev.d_tmp.as<char>();
        mc::EvScanDev d{};
        d.G = G, d.K = K, d.NP = static_cast<int>(NP), d.A = A, d.O = O;
        d.min_region = ev.min_region;
        d.gvert = D, d.gid = D + G, d.pvert = D + 2 * G, d.pvoid = d.pvert + K, d.pslot = d.pvoid + K;
        d.pscore = reinterpret_cast<const double *>(d.pslot + K);
        d.q_gt = d.pslot + 2 * K, d.q_pred = d.q_gt + NP, d.q_int = d.q_pred + NP;
        d.s_p0 = d.q_int + NP, d.s_p1 = d.s_p0 + A, d.s_nfilt = d.s_p1 + A, d.s_npred = d.s_nfilt + A, d.s_cls = d.s_npred + A;
        d.s_exoff = d.s_cls + A, d.s_cap = d.s_exoff + A;
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
        hipLaunchKernelGGL(mc::k_ev_greedy, dim3(ceil_div(U, 4)), dim3(256), 0, s, d);
        if (K) hipLaunchKernelGGL(mc::k_ev_fp, grid_for(static_cast<int64_t>(K) * O), dim3(256), 0, s, d);
        MC_HIP(hipGetLastError());
    }
    MC_HIP(hipStreamSynchronize(s));  // the upload reads this call's host words
    ctx->timer.collect();
    ev.ex_used += total;
    ev.units += U;
    ev.last = std::move(t);
    ev.have_last = true;
    ev.ap_valid = false;
    ev.runs_valid = false;
}

// the device half of mc_ev_add_scan*: every pointer is a device pointer
void ev_scan_device(mc_ctx *ctx, int64_t P, const int *gt, int K, const int64_t *off, int64_t npts, const int *pts,
                    const int *pcls, const double *pscore)
{
    EvState &ev = ctx->ev;
    hipStream_t s = ctx->stream;
    const int base = ev.class_ids[0] * 1000;
    ev.d_info.reserve(64);
    MC_HIP(hipMemsetAsync(ev.d_info.ptr, 0, 64, s));
    int info[4] = {0, 0, 0, 0};
    {
        TimedScope ts(ctx->timer, s, "ev_scan");
        hipLaunchKernelGGL(mc::k_ev_validate, grid_for(std::max<int64_t>(std::max(P, npts), K + 1)), dim3(256), 0, s, P, gt, K,
                           off, npts, pts, ev.no_class ? 1 : 0, base, ev.d_info.as<int>());
        MC_HIP(hipGetLastError());
    }
    MC_HIP(hipMemcpyAsync(info, ev.d_info.ptr, 8, hipMemcpyDeviceToHost, s));
    MC_HIP(hipStreamSynchronize(s));
    MC_REQUIRE(!(info[0] & 1), MC_ERR_INVALID, "negative ground-truth id");
    MC_REQUIRE(!(info[0] & 4), MC_ERR_INVALID, "prediction offsets must start at 0, ascend and end at num_pred_pts");
    MC_REQUIRE(!(info[0] & 2), MC_ERR_INVALID, "prediction point id out of range");
    const int R = info[1] + 1, C = ev.C;
    const size_t gcap = static_cast<size_t>(std::min<int64_t>(R, P)) + 1;
    ev.d_cnt.reserve(static_cast<size_t>(R) * 4);
    ev.d_inst.reserve(static_cast<size_t>(R) * 4);
    ev.d_tmp_id.reserve(gcap * 4);
    ev.d_class.reserve((3 * static_cast<size_t>(C) + 1) * 4);
    ev.d_gcls.reserve(gcap * 4);
    ev.d_gid.reserve(gcap * 4);
    ev.d_gvert.reserve(gcap * 8);
    ev.d_pinst.reserve(static_cast<size_t>(P) * 4 + 8);
    // per prediction: keep, class, pairs, kept-before, pairs-before (int), vert, void (int64)
    const size_t k8 = (static_cast<size_t>(K) * 4 + 7) & ~size_t(7);
    ev.d_pk.reserve(5 * k8 + 2 * static_cast<size_t>(K) * 8 + 8);
    ev.d_pair_gt.reserve(static_cast<size_t>(npts) * 4 + 8);
    ev.d_pair_int.reserve(static_cast<size_t>(npts) * 8 + 8);
    char *pk = ev.d_pk.as<char>();
    int *d_keep = reinterpret_cast<int *>(pk), *d_pcls = reinterpret_cast<int *>(pk + k8),
        *d_npair = reinterpret_cast<int *>(pk + 2 * k8), *d_kept = reinterpret_cast<int *>(pk + 3 * k8),
        *d_pbase = reinterpret_cast<int *>(pk + 4 * k8);
    int64_t *d_pvert = reinterpret_cast<int64_t *>(pk + 5 * k8), *d_pvoid = d_pvert + K;
    int *class_cnt = ev.d_class.as<int>(), *class_first = class_cnt + C, *class_off = class_first + C;
    // the compact tables as one run of words, sized by their bounds (instances, K predictions, npts pairs)
    ev.d_out.reserve((3 * gcap + 4 * static_cast<size_t>(K) + 3 * static_cast<size_t>(npts) + 1) * 8);
    MC_HIP(hipMemsetAsync(ev.d_cnt.ptr, 0, static_cast<size_t>(R) * 4, s));
    MC_HIP(hipMemsetAsync(ev.d_inst.ptr, 0xff, static_cast<size_t>(R) * 4, s));
    MC_HIP(hipMemsetAsync(class_cnt, 0, static_cast<size_t>(C) * 4, s));
    MC_HIP(hipMemsetAsync(class_first, 0x7f, static_cast<size_t>(C) * 4, s));
    {
        TimedScope ts(ctx->timer, s, "ev_scan");
        if (P && R <= mc::kEvCountLds)
            hipLaunchKernelGGL(mc::k_ev_gt_count_lds, grid_for(P, 2048, 256), dim3(256), 0, s, P, gt, ev.no_class ? 1 : 0, base, R,
                               ev.d_cnt.as<int>());
        else if (P)
            hipLaunchKernelGGL(mc::k_ev_gt_count, grid_for(P), dim3(256), 0, s, P, gt, ev.no_class ? 1 : 0, base,
                               ev.d_cnt.as<int>());
        hipLaunchKernelGGL(mc::k_ev_gt_table, dim3(1), dim3(1024), 0, s, R, ev.d_cnt.as<int>(), ev.d_lab2cls.as<int>(), ev.nlab,
                           C, ev.d_tmp_id.as<int>(), class_cnt, class_first, class_off, ev.d_gcls.as<int>(),
                           ev.d_gid.as<int>(), ev.d_gvert.as<int64_t>(), ev.d_inst.as<int>(), ev.d_info.as<int>() + 4);
        if (P)
            hipLaunchKernelGGL(mc::k_ev_point_inst, grid_for(P), dim3(256), 0, s, P, gt, ev.no_class ? 1 : 0, base,
                               ev.d_lab2cls.as<int>(), ev.nlab, ev.d_inst.as<int>(), ev.d_pinst.as<int>());
        if (K)
            hipLaunchKernelGGL(mc::k_ev_inter, dim3(std::min(K, 8192)), dim3(256), 0, s, K, off, pts, pcls, ev.no_class ? 1 : 0,
                               ev.d_lab2cls.as<int>(), ev.nlab, static_cast<int>(std::min<int64_t>(ev.min_region, INT32_MAX)),
                               ev.d_pinst.as<int>(), class_off, d_keep, d_pcls, d_pvert, d_pvoid, d_npair,
                               ev.d_pair_gt.as<int>(), ev.d_pair_int.as<int64_t>());
        hipLaunchKernelGGL(mc::k_ev_pred_scan, dim3(1), dim3(1024), 0, s, K, d_keep, d_npair, d_kept, d_pbase,
                           ev.d_info.as<int>() + 4);
        hipLaunchKernelGGL(mc::k_ev_compact, dim3(std::max(1, std::min(K, 8192))), dim3(256), 0, s, K, off, d_keep, d_kept, d_pbase,
                           d_npair, d_pcls, d_pvert, d_pvoid, pscore, ev.d_pair_gt.as<int>(), ev.d_pair_int.as<int64_t>(),
                           ev.d_gcls.as<int>(), ev.d_gid.as<int>(), ev.d_gvert.as<int64_t>(), ev.d_info.as<int>() + 4,
                           ev.d_out.as<int64_t>());
        MC_HIP(hipGetLastError());
    }
    MC_HIP(hipMemcpyAsync(info, ev.d_info.as<int>() + 4, 12, hipMemcpyDeviceToHost, s));
    MC_HIP(hipStreamSynchronize(s));
    const int G = info[0], Kk = info[1], NP = info[2];
    const size_t words = 3 * static_cast<size_t>(G) + 4 * static_cast<size_t>(Kk) + 3 * static_cast<size_t>(NP);
    ev.h_out.resize(words + 1);
    if (words) MC_HIP(hipMemcpyAsync(ev.h_out.data(), ev.d_out.ptr, words * 8, hipMemcpyDeviceToHost, s));
    MC_HIP(hipStreamSynchronize(s));
    ctx->timer.collect();
    const int64_t *w = ev.h_out.data();
    EvTables t;
    t.gcls.assign(w, w + G), t.gid.assign(w + G, w + 2 * G), t.gvert.assign(w + 2 * G, w + 3 * G);
    w += 3 * static_cast<size_t>(G);
    t.pcls.assign(w, w + Kk), t.pvert.assign(w + Kk, w + 2 * Kk), t.pvoid.assign(w + 2 * Kk, w + 3 * Kk);
    t.pscore.resize(Kk);
    if (Kk) std::memcpy(t.pscore.data(), w + 3 * static_cast<size_t>(Kk), static_cast<size_t>(Kk) * 8);
    w += 4 * static_cast<size_t>(Kk);
    t.ppred.assign(w, w + NP), t.pgt.assign(w + NP, w + 2 * NP), t.pint.assign(w + 2 * NP, w + 3 * NP);
    ev_commit(ctx, std::move(t));
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
constexpr int64_t kEvStateWord = (int64_t(1) << 32) | 0x5645434d;  // version 1, "MCEV"
constexpr size_t kEvStateHeader = 48;

struct EvLayout {  // byte offsets of the sections
    size_t ids, ov, roff, hf, fl, key, nt, nf, bytes;
};

EvLayout ev_layout(int C, int O, int64_t R)
{
    auto up = [](size_t b) { return (b + 7) & ~size_t(7); };
    const size_t NC = static_cast<size_t>(C) * O, r = static_cast<size_t>(R);
    EvLayout L;
    L.ids = kEvStateHeader;
    L.ov = L.ids + up(4 * static_cast<size_t>(C));
    L.roff = L.ov + 8 * static_cast<size_t>(O);
    L.hf = L.roff + 8 * (NC + 1);
    L.fl = L.hf + 8 * NC;
    L.key = L.fl + up(4 * NC);
    L.nt = L.key + 8 * r;
    L.nf = L.nt + up(4 * r);
    L.bytes = L.nf + up(4 * r);
    return L;
}

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
    const EvLayout L = ev_layout(C, O, R);
    std::vector<int64_t> head(L.roff / 8, 0);
    head[0] = kEvStateWord, head[1] = C, head[2] = O, head[3] = ev.min_region, head[4] = ev.no_class ? 1 : 0, head[5] = R;
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

void ev_merge(mc_ctx *ctx, const void *buf, int64_t bytes, bool on_device)
{
    EvState &ev = ctx->ev;
    hipStream_t s = ctx->stream;
    const int C = ev.C, O = ev.O, NC = C * O;
    MC_REQUIRE(buf && bytes >= static_cast<int64_t>(kEvStateHeader), MC_ERR_INVALID, "state buffer is truncated");
    MC_REQUIRE(!on_device || (reinterpret_cast<uintptr_t>(buf) & 7) == 0, MC_ERR_INVALID, "state buffer must be 8-byte aligned");
    const char *src = static_cast<const char *>(buf);
    auto take = [&](void *dst, size_t at, size_t n) {  // a part of the buffer to the host
        if (on_device) fetch(ctx, dst, src + at, n);
        else std::memcpy(dst, src + at, n);
    };
    int64_t hdr[6];
    take(hdr, 0, kEvStateHeader);
    MC_REQUIRE(hdr[0] == kEvStateWord, MC_ERR_INVALID, "not a state buffer of this version");
    MC_REQUIRE(hdr[1] == C && hdr[2] == O && hdr[3] == ev.min_region && hdr[4] == (ev.no_class ? 1 : 0), MC_ERR_INVALID,
               "state buffer of another configuration");
    const int64_t R = hdr[5];
    MC_REQUIRE(R >= 0 && R < (int64_t(1) << 31), MC_ERR_INVALID, "bad run count");
    const EvLayout L = ev_layout(C, O, R);
    MC_REQUIRE(static_cast<int64_t>(L.bytes) <= bytes, MC_ERR_INVALID, "state buffer is truncated");
    // configuration and per-cell sections on the host
    std::vector<int64_t> mid((L.key - L.ids) / 8);
    take(mid.data(), L.ids, L.key - L.ids);
    const char *mb = reinterpret_cast<const char *>(mid.data()) - L.ids;
    MC_REQUIRE(std::memcmp(mb + L.ids, ev.class_ids.data(), static_cast<size_t>(C) * 4) == 0 &&
                   std::memcmp(mb + L.ov, ev.overlaps.data(), static_cast<size_t>(O) * 8) == 0,
               MC_ERR_INVALID, "state buffer of another configuration");
    const int64_t *roff = reinterpret_cast<const int64_t *>(mb + L.roff), *hf = reinterpret_cast<const int64_t *>(mb + L.hf);
    const uint32_t *fl = reinterpret_cast<const uint32_t *>(mb + L.fl);
    MC_REQUIRE(roff[0] == 0 && roff[NC] == R, MC_ERR_INVALID, "run offsets must ascend from 0 to the run count");
    std::vector<int> cells;
    for (int c = 0; c < NC; c++) {
        MC_REQUIRE(roff[c + 1] >= roff[c], MC_ERR_INVALID, "run offsets must ascend from 0 to the run count");
        MC_REQUIRE(hf[c] >= 0, MC_ERR_INVALID, "negative hard false negative count");
        MC_REQUIRE(fl[c] <= 3u, MC_ERR_INVALID, "unknown flag bits");
        if (roff[c + 1] > roff[c]) cells.push_back(c);
    }
    const int U = static_cast<int>(cells.size());
    const char *D = src;
    if (!on_device) {
        ev.d_merge.reserve(L.bytes);
        MC_HIP(hipMemcpyAsync(ev.d_merge.ptr, src, L.bytes, hipMemcpyHostToDevice, s));
        D = ev.d_merge.as<char>();
    }
    const int64_t *d_roff = reinterpret_cast<const int64_t *>(D + L.roff), *d_hf = reinterpret_cast<const int64_t *>(D + L.hf);
    const unsigned *d_fl = reinterpret_cast<const unsigned *>(D + L.fl);
    const unsigned long long *d_key = reinterpret_cast<const unsigned long long *>(D + L.key);
    const unsigned *d_nt = reinterpret_cast<const unsigned *>(D + L.nt), *d_nf = reinterpret_cast<const unsigned *>(D + L.nf);
    // the run checks behind one flag word, and the examples of all runs
    ev.d_info.reserve(64);
    MC_HIP(hipMemsetAsync(ev.d_info.ptr, 0, 16, s));
    if (R) {
        TimedScope ts(ctx->timer, s, "ev_merge");
        hipLaunchKernelGGL(mc::k_ev_state_check, grid_for(R), dim3(256), 0, s, NC, R, d_roff, d_key, d_nt, d_nf,
                           ev.d_info.as<int>(), reinterpret_cast<unsigned long long *>(ev.d_info.as<char>() + 8));
        MC_HIP(hipGetLastError());
    }
    unsigned long long chk[2] = {0, 0};
    fetch(ctx, chk, ev.d_info.ptr, 16);
    const int bad = static_cast<int>(chk[0] & 0xffffffffu);
    MC_REQUIRE(!(bad & 1), MC_ERR_INVALID, "a run without examples");
    MC_REQUIRE(!(bad & 2), MC_ERR_INVALID, "a key that is no score (NaN)");
    MC_REQUIRE(!(bad & 4), MC_ERR_INVALID, "keys must ascend strictly within a cell");
    const unsigned long long total = chk[1];
    MC_REQUIRE(total < (1ull << 31) && ev.ex_used + static_cast<int64_t>(total) < (int64_t(1) << 31) &&
                   static_cast<int64_t>(ev.units) + U < (int64_t(1) << 31),
               MC_ERR_UNSUPPORTED, "more than 2^31 examples");
    // ---- from here on the accumulation changes ----
    const int64_t add = static_cast<int64_t>(total);
    ev_grow(ev.d_ex_key, ev.ex_used * 8, (ev.ex_used + add) * 8 + 8, s);
    ev_grow(ev.d_ex_true, ev.ex_used, ev.ex_used + add + 8, s);
    ev_grow(ev.d_unit_cell, static_cast<size_t>(ev.units) * 4, static_cast<size_t>(ev.units + U) * 4 + 8, s);
    ev_grow(ev.d_unit_cnt, static_cast<size_t>(ev.units) * 4, static_cast<size_t>(ev.units + U) * 4 + 8, s);
    ev_grow(ev.d_unit_off, static_cast<size_t>(ev.units) * 8, static_cast<size_t>(ev.units + U) * 8 + 8, s);
    ev.d_tmp.reserve(static_cast<size_t>(U) * 4 + 8);
    ev.d_words.reserve((static_cast<size_t>(R) + 1) * 4 + 8);
    if (U) MC_HIP(hipMemcpyAsync(ev.d_tmp.ptr, cells.data(), static_cast<size_t>(U) * 4, hipMemcpyHostToDevice, s));
    int *run_ex = ev.d_words.as<int>();
    {
        TimedScope ts(ctx->timer, s, "ev_merge");
        if (R) {
            hipLaunchKernelGGL(mc::k_ev_state_scan, dim3(1), dim3(1024), 0, s, static_cast<int>(R), d_nt, d_nf, run_ex);
            hipLaunchKernelGGL(mc::k_ev_state_expand, grid_for(add), dim3(256), 0, s, static_cast<int>(R), run_ex, d_key, d_nt,
                               ev.d_ex_key.as<unsigned long long>() + ev.ex_used, ev.d_ex_true.as<unsigned char>() + ev.ex_used);
        }
        hipLaunchKernelGGL(mc::k_ev_state_units, grid_for(std::max(NC, U)), dim3(256), 0, s, NC, U, ev.d_tmp.as<int>(), d_roff,
                           run_ex, d_hf, d_fl, ev.ex_used, ev.d_unit_cell.as<int>() + ev.units, ev.d_unit_cnt.as<int>() + ev.units,
                           ev.d_unit_off.as<int64_t>() + ev.units, ev.d_hardfn.as<unsigned long long>(),
                           ev.d_flags.as<unsigned>());
        MC_HIP(hipGetLastError());
    }
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
            ev_scan_device(ctx, num_points, gt_ids, num_pred, pred_off, num_pred_pts, pred_pts, pred_classes, pred_scores);
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
        ev_scan_device(ctx, num_points, ev.d_in[0].as<int>(), num_pred, ev.d_in[1].as<int64_t>(), num_pred_pts,
                       ev.d_in[2].as<int>(), pred_classes ? ev.d_in[3].as<int>() : nullptr,
                       pred_scores ? ev.d_in[4].as<double>() : nullptr);
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
        ev_scan_device(ctx, P, gt, nf, pp.d_opoff.as<int64_t>(), np, pp.d_opts.as<int>(), nullptr, nullptr);
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
        ev_merge(ctx, buf, bytes, on_device != 0);
    });
}

}  // extern "C"
