// mc_pp_host.inl — post-processing (utils/post_process.py:173-194): the host side (included by
// mc_api.hip, same translation unit).  pp_run drives one call over a PPRun, the sizes, device inputs
// and scratch arrays of the call: pp_layout (checks and per-node layout), pp_dbscan, pp_filter, the
// keep decision, pp_merge, pp_publish; the decisions between the kernels are mc_pp_plan.hpp's.  The
// three public entries check their arguments, put every array on the device and call it.
namespace {

static_assert(sizeof(mc::PPInt2) == sizeof(int2), "mc::PPInt2 is copied to and from the kernels' int2 lists");

// an array (of the host, unless `kind` says otherwise) into a device buffer of the call or of the context
void pp_upload(hipStream_t s, DevBuf &b, const void *src, size_t bytes, hipMemcpyKind kind = hipMemcpyHostToDevice)
{
    b.reserve(bytes + 8);
    if (bytes) MC_HIP(hipMemcpyAsync(b.ptr, src, bytes, kind, s));
}

// One post-processing run: the sizes and the input arrays on the device (a; the node arrays are the
// context's own d_pp_* buffers, which the export reads later), the kernel parameters, what the steps
// bring to the host, and the scratch arrays they hand to each other, freed when the run ends.
struct PPRun {
    mc::PPArgs a{};
    mc::PPDev pr{};
    int64_t H = 0;                      // hit-bit words of all nodes
    std::vector<int64_t> h_npoff;       // node point offsets
    std::vector<int32_t> h_order;       // the size order
    std::vector<int32_t> h_nm, h_nv;    // masks and points each object kept (k_pp_filter)
    std::vector<double> h_box;          // the objects' boxes
    DevBuf qfp, hitw, hoff, nsize, dorder, flag;                                                          // pp_layout
    DevBuf xyz, pcell, pbkt, bcnt, bstart, blist, ncnt, par, root, rnk, lab, ccnt, nob, nsh, tick, skey, sxyz, sidx, obase;  // pp_dbscan
    DevBuf hit, cvid, qobj, qcov, onm, onv, obox, eobj;                                                   // pp_filter
    DevBuf dk, pcnt, plist, mxc, inter, dbox, dlen, dec, inv, nl, lst;                                    // pp_merge
};

// entry_object / mask_object / mask_coverage on the host (mc_pp_get_results)
void pp_fetch_host(mc_ctx *ctx)
{
    PpState &pp = ctx->pp;
    if (pp.host) return;
    hipStream_t s = ctx->stream;
    const int64_t E = pp.info.num_entries, Q = pp.info.num_node_masks;
    pp.entry_obj.resize(E);
    pp.qobj.resize(Q);
    pp.qcov.resize(Q);
    if (E) MC_HIP(hipMemcpyAsync(pp.entry_obj.data(), pp.d_eobj.ptr, E * 4, hipMemcpyDeviceToHost, s));
    if (Q) {
        MC_HIP(hipMemcpyAsync(pp.qobj.data(), pp.d_qobj.ptr, Q * 4, hipMemcpyDeviceToHost, s));
        MC_HIP(hipMemcpyAsync(pp.qcov.data(), pp.d_qcov.ptr, Q * 8, hipMemcpyDeviceToHost, s));
    }
    MC_HIP(hipStreamSynchronize(s));
    ctx->timer.collect();
    for (auto &o : pp.entry_obj)
        if (o >= 0 && pp.state[o] != 2) o = -1;
    pp.host = true;
}

// dbscan_process: the nodes above big_min points (the first nbig of the size order) split over the chip,
// the others a workgroup each.  Returns the nodes' object bases (the last is K), also put in r.obase.
std::vector<int32_t> pp_dbscan(mc_ctx *ctx, PPRun &r)
{
    hipStream_t s = ctx->stream;
    const mc::PPArgs &a = r.a;
    const int N = a.N;
    const int64_t E = a.E;
    r.skey.reserve(E * 8 + 8);  // bucket-ordered copies of the cell keys, points and indices
    r.sxyz.reserve(E * 24 + 8);
    r.sidx.reserve(E * 4 + 8);
    r.xyz.reserve(E * 24 + 8);
    r.pcell.reserve(E * 8 + 8);
    for (DevBuf *b : {&r.pbkt, &r.blist, &r.ncnt, &r.par, &r.root, &r.rnk, &r.lab}) b->reserve(E * 4 + 8);
    r.bcnt.reserve((2 * E + N + 1) * 4);
    r.bstart.reserve((2 * E + N + 1) * 4);
    r.ccnt.reserve((E + N + 1) * 4);
    r.nob.reserve(N * 4 + 8);
    r.nsh.reserve(N * 4 + 8);
    r.tick.reserve(16);
    MC_HIP(hipMemsetAsync(r.bcnt.ptr, 0, (2 * E + N + 1) * 4, s));
    MC_HIP(hipMemsetAsync(r.tick.ptr, 0, 16, s));
    {
        mc::TimedScope ts(ctx->timer, s, "pp_dbscan");
        if (E) hipLaunchKernelGGL(mc::k_pp_gather, grid_for(3 * E), dim3(256), 0, s, a.scene, a.npts, E, r.xyz.as<double>());
        int big_min = mc::kPPLdsUF;
        if (const char *e = getenv("MC_PP_BIG_MIN")) big_min = std::max(1, atoi(e));
        std::vector<mc::PPInt2> items;
        const int nbig = mc::pp_big_items(r.h_npoff.data(), r.h_order.data(), N, big_min, items);
        mc::PPNodes b{a.npoff, r.xyz.as<double>(), r.pcell.as<unsigned long long>(), r.pbkt.as<int>(), r.bcnt.as<int>(),
                      r.bstart.as<int>(), r.blist.as<int>(), r.ncnt.as<int>(), r.par.as<int>(), r.root.as<int>(),
                      r.rnk.as<int>(), r.lab.as<int>(), r.ccnt.as<int>(), r.nob.as<int>(), r.nsh.as<int>(), nullptr,
                      r.skey.as<unsigned long long>(), r.sxyz.as<double>(), r.sidx.as<int>()};
        if (nbig) {
            DevBuf ditems, gcm;
            pp_upload(s, ditems, items.data(), items.size() * sizeof(int2));
            gcm.reserve(static_cast<size_t>(N) * 12 + 8);
            b.gcm = gcm.as<int>();
            const int ni = static_cast<int>(items.size());
            hipLaunchKernelGGL(mc::k_pp_big_grid<512>, dim3(nbig), dim3(512), 0, s, nbig, r.dorder.as<int>(), r.pr, b);
            hipLaunchKernelGGL((mc::k_pp_big_walk<512, 0>), dim3(std::min(ni, 65536)), dim3(512), 0, s, ni,
                               ditems.as<int2>(), r.pr, b);
            hipLaunchKernelGGL((mc::k_pp_big_walk<512, 1>), dim3(std::min(ni, 65536)), dim3(512), 0, s, ni,
                               ditems.as<int2>(), r.pr, b);
            hipLaunchKernelGGL(mc::k_pp_big_label<512>, dim3(nbig), dim3(512), 0, s, nbig, r.dorder.as<int>(), r.pr, b);
            MC_HIP(hipGetLastError());
            MC_HIP(hipStreamSynchronize(s));  // ditems / gcm are freed at scope exit
            b.gcm = nullptr;                  // (k_pp_dbscan keeps cmax in registers)
        }
        if (N > nbig)  // 512-thread workgroups (1024 spills the neighbour walks)
            hipLaunchKernelGGL(mc::k_pp_dbscan<512>, dim3(std::max(1, std::min(N - nbig, ctx->num_cu * 2))), dim3(512), 0, s,
                               N - nbig, r.dorder.as<int>() + nbig, r.tick.as<int>(), r.pr, b);
        MC_HIP(hipGetLastError());
    }
    std::vector<int32_t> h_nob(N), base(N + 1, 0);
    if (N) MC_HIP(hipMemcpyAsync(h_nob.data(), r.nob.ptr, N * 4, hipMemcpyDeviceToHost, s));
    MC_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < N; k++) base[k + 1] = base[k] + h_nob[k];
    pp_upload(s, r.obase, base.data(), static_cast<size_t>(N + 1) * 4);
    return base;
}

// filter_point of the K objects; the per-object counts and boxes come to the host
void pp_filter(mc_ctx *ctx, PPRun &r, int K)
{
    PpState &pp = ctx->pp;
    hipStream_t s = ctx->stream;
    const mc::PPArgs &a = r.a;
    const int N = a.N;
    const int64_t P = a.P, E = a.E, Q = a.Q, H = r.H;
    const int slots = std::max(1, std::min(N, ctx->num_cu));
    if (pp.posmap_P < P || pp.posmap_slots < slots) {
        pp.d_posmap.release();
        pp.d_posmap.reserve(static_cast<size_t>(slots) * P * 4 + 8);
        MC_HIP(hipMemsetAsync(pp.d_posmap.ptr, 0xFF, static_cast<size_t>(slots) * P * 4, s));
        pp.posmap_P = P;
        pp.posmap_slots = slots;
    }
    r.hit.reserve(H * 8 + 8);
    r.cvid.reserve(E * 4 + 8);
    r.qobj.reserve(Q * 4 + 8);
    r.qcov.reserve(Q * 8 + 8);
    r.onm.reserve(K * 4 + 8);
    r.onv.reserve(K * 4 + 8);
    r.obox.reserve(K * 48 + 8);
    r.eobj.reserve(E * 4 + 8);
    if (H) MC_HIP(hipMemsetAsync(r.hit.ptr, 0, H * 8, s));
    if (K) MC_HIP(hipMemsetAsync(r.onm.ptr, 0, K * 4, s));
    {
        mc::TimedScope ts(ctx->timer, s, "pp_filter");
        if (N) hipLaunchKernelGGL(mc::k_pp_filter, dim3(slots), dim3(256), 0, s, N, r.dorder.as<int>(), r.tick.as<int>() + 1,
                                  r.pr, a.FW, P, a.npoff, a.npts, a.nvf, r.hoff.as<int64_t>(), a.qoff, a.qm, r.qfp.as<int>(),
                                  a.mask_off, a.mask_pts, a.pfm, r.xyz.as<double>(), r.lab.as<int>(), r.ccnt.as<int>(),
                                  r.nob.as<int>(), r.nsh.as<int>(), r.obase.as<int>(), pp.d_posmap.as<int>(),
                                  r.hit.as<unsigned long long>(), r.cvid.as<int>(), r.qobj.as<int>(), r.qcov.as<double>(),
                                  r.onm.as<int>(), r.onv.as<int>(), r.obox.as<double>(), r.eobj.as<int>());
        MC_HIP(hipGetLastError());
    }
    r.h_nm.resize(K);
    r.h_nv.resize(K);
    r.h_box.resize(static_cast<size_t>(K) * 6);
    if (K) {
        MC_HIP(hipMemcpyAsync(r.h_nm.data(), r.onm.ptr, K * 4, hipMemcpyDeviceToHost, s));
        MC_HIP(hipMemcpyAsync(r.h_nv.data(), r.onv.ptr, K * 4, hipMemcpyDeviceToHost, s));
        MC_HIP(hipMemcpyAsync(r.h_box.data(), r.obox.ptr, K * 48, hipMemcpyDeviceToHost, s));
    }
    MC_HIP(hipStreamSynchronize(s));
}

// merge_overlapping_objects: the objects per point (k_pp_index, redone once with the slots the fullest
// point asked for), the pair intersections, the decisions, and the greedy pass over them, on the host
// when the non-zero decisions fit the list.  Returns the invalid flag of each kept object.
std::vector<uint8_t> pp_merge(mc_ctx *ctx, PPRun &r, int K, const mc::PPKept &kept)
{
    hipStream_t s = ctx->stream;
    const mc::PPArgs &a = r.a;
    const int64_t P = a.P, E = a.E;
    const int Kk = static_cast<int>(kept.kept.size());
    std::vector<uint8_t> h_inv(Kk, 0);
    if (Kk <= 1) return h_inv;
    mc::TimedScope ts(ctx->timer, s, "pp_merge");
    pp_upload(s, r.dk, kept.kidx.data(), static_cast<size_t>(K) * 4);
    pp_upload(s, r.dbox, kept.kbox.data(), static_cast<size_t>(Kk) * 48);
    pp_upload(s, r.dlen, kept.klen.data(), static_cast<size_t>(Kk) * 4);
    r.pcnt.reserve(P * 4 + 8);
    r.mxc.reserve(8);
    int sl = mc::kPPSlots;
    for (int pass = 0; pass < 2; pass++) {
        r.plist.reserve(static_cast<size_t>(P) * sl * 4 + 8);
        MC_HIP(hipMemsetAsync(r.pcnt.ptr, 0, P * 4, s));
        MC_HIP(hipMemsetAsync(r.mxc.ptr, 0, 4, s));
        hipLaunchKernelGGL(mc::k_pp_index, grid_for(E), dim3(256), 0, s, E, a.npts, r.eobj.as<int>(), r.dk.as<int>(), sl,
                           r.pcnt.as<int>(), r.plist.as<int>(), r.mxc.as<int>());
        int mx = 0;
        MC_HIP(hipMemcpyAsync(&mx, r.mxc.ptr, 4, hipMemcpyDeviceToHost, s));
        MC_HIP(hipStreamSynchronize(s));
        if (mx <= sl) break;
        sl = mx;
    }
    r.inter.reserve(static_cast<size_t>(Kk) * Kk * 4);
    r.dec.reserve(static_cast<size_t>(Kk) * Kk);
    r.inv.reserve(Kk + 8);
    MC_HIP(hipMemsetAsync(r.inter.ptr, 0, static_cast<size_t>(Kk) * Kk * 4, s));
    hipLaunchKernelGGL(mc::k_pp_pairs, grid_for(P), dim3(256), 0, s, P, sl, r.pcnt.as<int>(), r.plist.as<int>(), Kk,
                       r.inter.as<int>());
    int kCap = 1 << 16;  // non-zero decisions handled by the host pass; more: k_pp_greedy
    if (const char *e = getenv("MC_PP_GREEDY_CAP")) kCap = std::max(0, atoi(e));  // tests force the device pass
    r.nl.reserve(8);
    r.lst.reserve(static_cast<size_t>(std::max(kCap, 1)) * sizeof(int2));
    MC_HIP(hipMemsetAsync(r.nl.ptr, 0, 4, s));
    hipLaunchKernelGGL(mc::k_pp_decide, grid_for(static_cast<int64_t>(Kk) * Kk), dim3(256), 0, s, Kk, r.pr,
                       r.dbox.as<double>(), r.dlen.as<int>(), r.inter.as<int>(), r.dec.as<unsigned char>(), kCap,
                       r.nl.as<int>(), r.lst.as<int2>());
    MC_HIP(hipGetLastError());
    int nd = 0;
    MC_HIP(hipMemcpyAsync(&nd, r.nl.ptr, 4, hipMemcpyDeviceToHost, s));
    MC_HIP(hipStreamSynchronize(s));
    if (nd <= kCap) {
        std::vector<mc::PPInt2> d(nd);
        if (nd) MC_HIP(hipMemcpy(d.data(), r.lst.ptr, static_cast<size_t>(nd) * sizeof(int2), hipMemcpyDeviceToHost));
        mc::pp_greedy_merge(d, h_inv);
    } else {
        hipLaunchKernelGGL(mc::k_pp_greedy, dim3(1), dim3(1024), 0, s, Kk, r.dec.as<unsigned char>(), r.inv.as<unsigned char>());
        MC_HIP(hipGetLastError());
        MC_HIP(hipMemcpyAsync(h_inv.data(), r.inv.ptr, Kk, hipMemcpyDeviceToHost, s));
        MC_HIP(hipStreamSynchronize(s));  // h_inv is pageable host memory read by the caller
    }
    return h_inv;
}

// The result into the context; the per-entry device results are swapped in for the export, and
// host_results also brings them to the host (mc_pp_run), else they stay on the device until asked for
void pp_publish(mc_ctx *ctx, PPRun &r, const std::vector<int32_t> &base, const mc::PPKept &kept,
                const std::vector<uint8_t> &inv, bool host_results)
{
    PpState &pp = ctx->pp;
    const int N = r.a.N, K = base[N], Kk = static_cast<int>(kept.kept.size());
    pp.state.assign(K, 0);
    int nfin = 0;
    for (int i = 0; i < Kk; i++) {
        pp.state[kept.kept[i]] = inv[i] ? 1 : 2;
        nfin += inv[i] ? 0 : 1;
    }
    pp.obj_node.resize(K);
    for (int k = 0; k < N; k++)
        for (int o = base[k]; o < base[k + 1]; o++) pp.obj_node[o] = k;
    pp.info = {K, Kk, nfin, r.a.E, r.a.Q};  // objects, filtered, final, entries, node masks
    mc::pp_final_tables(pp.state, pp.obj_node, r.h_nv.data(), r.h_nm.data(), pp.fslot, pp.fin,
                        pp.fin_node, pp.opoff, pp.omoff);
    pp.box = std::move(r.h_box);
    pp.d_eobj.swap(r.eobj);
    pp.d_qobj.swap(r.qobj);
    pp.d_qcov.swap(r.qcov);
    pp.P = r.a.P;
    pp.F = r.a.F;
    pp.host = pp.have_export = false;
    if (host_results) pp_fetch_host(ctx);
    else {
        MC_HIP(hipStreamSynchronize(ctx->stream));
        ctx->timer.collect();
    }
    pp.have = true;
}

// ---- the checked entry path ----
// (Defined after the steps above: template kernels are emitted in the order of their first use, and
// this order keeps the device code byte-identical to the build before the split, scripts/isa_diff.py.)
// first and last entry of the node point, node mask and mask offsets, read back from the device
void pp_read_ends(mc_ctx *ctx, const int64_t *const offs[3], const int lens[3], int64_t ends[6])
{
    for (int i = 0; i < 3; i++) {
        MC_HIP(hipMemcpyAsync(&ends[2 * i], offs[i], 8, hipMemcpyDeviceToHost, ctx->stream));
        MC_HIP(hipMemcpyAsync(&ends[2 * i + 1], offs[i] + lens[i], 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    MC_HIP(hipStreamSynchronize(ctx->stream));
}

// The O(1) checks of an entry's arguments in r.a, with E, Q and MP from the ends of the three offset
// arrays: host arrays (mc_pp_run, every array still the caller's), else read back
void pp_check_args(mc_ctx *ctx, const mc_pp_params *params, PPRun &r, bool host_arrays)
{
    mc::PPArgs &a = r.a;
    MC_REQUIRE(params, MC_ERR_INVALID, "null params");
    MC_REQUIRE(a.P >= 0 && a.P < (1ll << 31) && a.F >= 0 && a.Mt >= 0 && a.N >= 0, MC_ERR_INVALID, "bad sizes");
    MC_REQUIRE(a.F <= 16384, MC_ERR_UNSUPPORTED, "num_frames must be <= 16384");
    MC_REQUIRE(params->dbscan_eps > 0 && params->dbscan_min_points >= 1, MC_ERR_INVALID, "bad DBSCAN parameters");
    MC_REQUIRE(a.mask_off && a.npoff && a.qoff, MC_ERR_INVALID, "null offsets");
    const int64_t *const offs[3] = {a.npoff, a.qoff, a.mask_off};
    const int lens[3] = {a.N, a.N, a.Mt};
    int64_t ends[6];
    if (host_arrays)
        for (int i = 0; i < 3; i++) ends[2 * i] = offs[i][0], ends[2 * i + 1] = offs[i][lens[i]];
    else pp_read_ends(ctx, offs, lens, ends);
    MC_REQUIRE(ends[0] == 0 && ends[2] == 0 && ends[4] == 0, MC_ERR_INVALID, "offsets must start at 0");
    a.E = ends[1], a.Q = ends[3], a.MP = ends[5];
    MC_REQUIRE(a.E >= 0 && a.Q >= 0 && a.MP >= 0, MC_ERR_INVALID, "offsets must be ascending");
    MC_REQUIRE(a.E < (1ll << 30) && a.Q < (1ll << 31), MC_ERR_UNSUPPORTED, "too many node points");
    MC_REQUIRE((a.P == 0 || (a.scene && a.pfm)) && (a.E == 0 || a.npts) && (a.Q == 0 || (a.qm && a.qcol)) &&
                   (a.MP == 0 || a.mask_pts) && (a.N == 0 || a.nvf),
               MC_ERR_INVALID, "null argument");
    a.FW = (a.F + 63) / 64;
    r.pr = {params->dbscan_eps * params->dbscan_eps, params->dbscan_eps * 1.01, params->point_filter_threshold,
            params->overlapping_ratio, params->dbscan_min_points};  // eps2, ce (the cell edge), thr, ratio, minpts
}

// The checks of the arrays' contents and the per-node layout, as kernels behind one flag: ranges, each
// mask's frame rank among its node's visible frames, hit-bit words and extent per node, the size order.
// The host reads the flag, then the node offsets, the order and the hit-word total (O(num_nodes)).
void pp_layout(mc_ctx *ctx, PPRun &r)
{
    hipStream_t s = ctx->stream;
    const mc::PPArgs &a = r.a;
    const int N = a.N;
    r.qfp.reserve(a.Q * 4 + 8);
    r.hitw.reserve(static_cast<size_t>(N) * 8 + 8);
    r.hoff.reserve(static_cast<size_t>(N + 1) * 8);
    r.nsize.reserve(static_cast<size_t>(N) * 4 + 8);
    r.dorder.reserve(static_cast<size_t>(N) * 4 + 8);
    r.flag.reserve(8);
    MC_HIP(hipMemsetAsync(r.flag.ptr, 0, 4, s));
    {
        mc::TimedScope ts(ctx->timer, s, "pp_prep");
        hipLaunchKernelGGL(mc::k_pp_validate, grid_for(std::max<int64_t>(std::max(a.E, a.MP), std::max<int64_t>(a.Q, std::max(N, a.Mt)))),
                           dim3(256), 0, s, a, r.flag.as<int>());
        if (N) {
            hipLaunchKernelGGL(mc::k_pp_prep, dim3(std::min(N, 4096)), dim3(256), 0, s, a, r.pr, r.flag.as<int>(),
                               r.qfp.as<int>(), r.hitw.as<int64_t>(), r.nsize.as<int>());
            hipLaunchKernelGGL(mc::k_pp_order, grid_for(N), dim3(256), 0, s, N, r.nsize.as<int>(), r.flag.as<int>(),
                               r.dorder.as<int>());
        }
        hipLaunchKernelGGL(mc::k_pp_scan64<int64_t>, dim3(1), dim3(1024), 0, s, r.hitw.as<int64_t>(), N, r.hoff.as<int64_t>());
        MC_HIP(hipGetLastError());
    }
    int h_flag = 0;
    MC_HIP(hipMemcpyAsync(&h_flag, r.flag.ptr, 4, hipMemcpyDeviceToHost, s));
    MC_HIP(hipStreamSynchronize(s));
    MC_REQUIRE(!(h_flag & mc::kPPBadOffsets), MC_ERR_INVALID, "offsets must be ascending");
    MC_REQUIRE(!(h_flag & mc::kPPBadIndex), MC_ERR_INVALID, "a point, mask or frame index is out of range");
    MC_REQUIRE(!(h_flag & mc::kPPBadFrame), MC_ERR_INVALID,
               "a mask's frame is not among the node's visible frames (post_process.py:69 IndexError)");
    MC_REQUIRE(!(h_flag & mc::kPPTooWide), MC_ERR_UNSUPPORTED,
               "a node spans more than 2^21 DBSCAN cells per axis (eps too small)");
    r.h_npoff.assign(N + 1, 0);
    r.h_order.resize(std::max(N, 1));
    MC_HIP(hipMemcpyAsync(r.h_npoff.data(), a.npoff, static_cast<size_t>(N + 1) * 8, hipMemcpyDeviceToHost, s));
    if (N) MC_HIP(hipMemcpyAsync(r.h_order.data(), r.dorder.ptr, static_cast<size_t>(N) * 4, hipMemcpyDeviceToHost, s));
    MC_HIP(hipMemcpyAsync(&r.H, r.hoff.as<int64_t>() + N, 8, hipMemcpyDeviceToHost, s));
    MC_HIP(hipStreamSynchronize(s));
}

// dbscan_process, filter_point and merge_overlapping_objects of the nodes in r.a (pp_check_args passed,
// every array on the device, the node arrays in the context's d_pp_* buffers)
void pp_run(mc_ctx *ctx, PPRun &r, bool host_results)
{
    pp_layout(ctx, r);
    const std::vector<int32_t> base = pp_dbscan(ctx, r);
    const int K = base[r.a.N];
    pp_filter(ctx, r, K);
    const mc::PPKept kept = mc::pp_kept_objects(K, r.h_nv.data(), r.h_nm.data(), r.h_box.data());
    MC_REQUIRE(kept.kept.size() <= static_cast<size_t>(mc::kPPMaxKept), MC_ERR_UNSUPPORTED,
               "more than 46340 objects after filter_point");
    const std::vector<uint8_t> inv = pp_merge(ctx, r, K, kept);
    pp_publish(ctx, r, base, kept, inv, host_results);
}

// the export arrays of the last post-processing result, built once per result
void pp_build_export(mc_ctx *ctx)
{
    PpState &pp = ctx->pp;
    if (pp.have_export) return;
    hipStream_t s = ctx->stream;
    const int K = pp.info.num_objects, nf = pp.info.num_final;
    const int64_t np = pp.opoff[nf], nm = pp.omoff[nf];
    pp_upload(s, pp.d_fslot, pp.fslot.data(), static_cast<size_t>(K) * 4);
    pp_upload(s, pp.d_finobj, pp.fin.data(), static_cast<size_t>(nf) * 4);
    pp_upload(s, pp.d_finnode, pp.fin_node.data(), static_cast<size_t>(nf) * 4);
    pp_upload(s, pp.d_opoff, pp.opoff.data(), static_cast<size_t>(nf + 1) * 8);
    pp_upload(s, pp.d_omoff, pp.omoff.data(), static_cast<size_t>(nf + 1) * 8);
    pp.d_opts.reserve(np * 4 + 8);
    pp.d_omask.reserve(nm * 4 + 8);
    pp.d_ocov.reserve(nm * 8 + 8);
    pp.d_repre.reserve(static_cast<size_t>(nf) * 20 + 8);
    if (nf) {
        mc::TimedScope ts(ctx->timer, s, "pp_export");
        hipLaunchKernelGGL(mc::k_pp_ex_fill, dim3(std::min(nf, 4096)), dim3(256), 0, s, nf, pp.d_finobj.as<int>(),
                           pp.d_finnode.as<int>(), pp.d_npoff.as<int64_t>(), pp.d_npts.as<int>(),
                           pp.d_eobj.as<int>(), pp.d_qoff.as<int64_t>(), pp.d_qm.as<int>(),
                           pp.d_qobj.as<int>(), pp.d_qcov.as<double>(), pp.d_opoff.as<int64_t>(),
                           pp.d_opts.as<int>(), pp.d_omoff.as<int64_t>(), pp.d_omask.as<int>(),
                           pp.d_ocov.as<double>());
        hipLaunchKernelGGL(mc::k_pp_ex_repre, dim3(std::min(ceil_div(nf, 4), 4096)), dim3(256), 0, s, nf,
                           pp.d_omoff.as<int64_t>(), pp.d_ocov.as<double>(), pp.d_repre.as<int>());
        MC_HIP(hipGetLastError());
    }
    MC_HIP(hipStreamSynchronize(s));  // the uploads read the context's host vectors
    ctx->timer.collect();
    pp.have_export = true;
}

}  // namespace

extern "C" {

int mc_pp_run(mc_ctx *ctx, const mc_pp_params *params, int64_t num_points, int32_t num_frames, const double *scene_xyz,
              const uint64_t *pfm_bits, int32_t num_masks, const int64_t *mask_off, const int32_t *mask_pts,
              int32_t num_nodes, const uint64_t *node_vf_bits, const int64_t *node_pt_off, const int32_t *node_pts,
              const int64_t *node_mask_off, const int32_t *node_masks, const int32_t *node_mask_col)
{
    return guarded(ctx, [&] {
        PpState &pp = ctx->pp;
        pp.have = false;
        PPRun r;
        mc::PPArgs &a = r.a;  // the host arrays for the checks, then their device copies
        a.P = num_points, a.F = num_frames, a.Mt = num_masks, a.N = num_nodes;
        a.scene = scene_xyz;
        a.pfm = reinterpret_cast<const unsigned long long *>(pfm_bits);
        a.nvf = reinterpret_cast<const unsigned long long *>(node_vf_bits);
        a.mask_off = mask_off, a.npoff = node_pt_off, a.qoff = node_mask_off;
        a.mask_pts = mask_pts, a.npts = node_pts, a.qm = node_masks, a.qcol = node_mask_col;
        pp_check_args(ctx, params, r, true);
        hipStream_t s = ctx->stream;
        DevBuf scene, pfm, moff, mpts, nvf, qcol;
        pp_upload(s, scene, scene_xyz, static_cast<size_t>(a.P) * 24);
        pp_upload(s, pfm, pfm_bits, static_cast<size_t>(a.P) * a.FW * 8);
        pp_upload(s, moff, mask_off, static_cast<size_t>(a.Mt + 1) * 8);
        pp_upload(s, mpts, mask_pts, static_cast<size_t>(a.MP) * 4);
        pp_upload(s, pp.d_npoff, node_pt_off, static_cast<size_t>(a.N + 1) * 8);
        pp_upload(s, pp.d_npts, node_pts, static_cast<size_t>(a.E) * 4);
        pp_upload(s, nvf, node_vf_bits, static_cast<size_t>(a.N) * a.FW * 8);
        pp_upload(s, pp.d_qoff, node_mask_off, static_cast<size_t>(a.N + 1) * 8);
        pp_upload(s, pp.d_qm, node_masks, static_cast<size_t>(a.Q) * 4);
        pp_upload(s, qcol, node_mask_col, static_cast<size_t>(a.Q) * 4);
        a.scene = scene.as<double>();
        a.pfm = pfm.as<unsigned long long>(), a.nvf = nvf.as<unsigned long long>();
        a.mask_off = moff.as<int64_t>(), a.npoff = pp.d_npoff.as<int64_t>(), a.qoff = pp.d_qoff.as<int64_t>();
        a.mask_pts = mpts.as<int>(), a.npts = pp.d_npts.as<int>(), a.qm = pp.d_qm.as<int>();
        a.qcol = qcol.as<int>();
        pp_run(ctx, r, true);
        pp.d_qcol.swap(qcol);
    });
}

int mc_pp_run_device(mc_ctx *ctx, const mc_pp_params *params, int64_t num_points, int32_t num_frames,
                     const double *scene_xyz, const uint64_t *pfm_bits, int32_t num_masks, const int64_t *mask_off,
                     const int32_t *mask_pts, int32_t num_nodes, const uint64_t *node_vf_bits,
                     const int64_t *node_pt_off, const int32_t *node_pts, const int64_t *node_mask_off,
                     const int32_t *node_masks, const int32_t *node_mask_col)
{
    return guarded(ctx, [&] {
        PpState &pp = ctx->pp;
        pp.have = false;
        PPRun r;
        mc::PPArgs &a = r.a;
        a.P = num_points, a.F = num_frames, a.Mt = num_masks, a.N = num_nodes;
        a.scene = scene_xyz;
        a.pfm = reinterpret_cast<const unsigned long long *>(pfm_bits);
        a.nvf = reinterpret_cast<const unsigned long long *>(node_vf_bits);
        a.mask_off = mask_off, a.npoff = node_pt_off, a.qoff = node_mask_off;
        a.mask_pts = mask_pts, a.npts = node_pts, a.qm = node_masks, a.qcol = node_mask_col;
        pp_check_args(ctx, params, r, false);
        hipStream_t s = ctx->stream;  // the node arrays stay with the context for the export
        pp_upload(s, pp.d_npoff, a.npoff, static_cast<size_t>(a.N + 1) * 8, hipMemcpyDeviceToDevice);
        pp_upload(s, pp.d_npts, a.npts, static_cast<size_t>(a.E) * 4, hipMemcpyDeviceToDevice);
        pp_upload(s, pp.d_qoff, a.qoff, static_cast<size_t>(a.N + 1) * 8, hipMemcpyDeviceToDevice);
        pp_upload(s, pp.d_qm, a.qm, static_cast<size_t>(a.Q) * 4, hipMemcpyDeviceToDevice);
        pp_upload(s, pp.d_qcol, a.qcol, static_cast<size_t>(a.Q) * 4, hipMemcpyDeviceToDevice);
        a.npoff = pp.d_npoff.as<int64_t>(), a.npts = pp.d_npts.as<int>();
        a.qoff = pp.d_qoff.as<int64_t>(), a.qm = pp.d_qm.as<int>();
        a.qcol = pp.d_qcol.as<int>();
        pp_run(ctx, r, false);
    });
}

int mc_pp_run_clustered(mc_ctx *ctx, const mc_pp_params *params, const double *scene_xyz, int scene_on_device)
{
    return guarded(ctx, [&] {
        SceneState &sc = ctx->scene;
        GraphState &gr = ctx->graph;
        ClusterState &cl = ctx->cluster;
        PpState &pp = ctx->pp;
        pp.have = false;
        MC_REQUIRE(cl.have, MC_ERR_STATE, "no clustering result (mc_cluster_run first)");
        MC_REQUIRE(gr.nodes_from_graph, MC_ERR_STATE, "the nodes were given by mc_nodes_set: no mask table");
        MC_REQUIRE(!sharded(ctx) || ctx->shard.pending == 0, MC_ERR_STATE, "this rank does not hold the full result");
        MC_REQUIRE(scene_xyz || (ctx->bp.have_points && ctx->bp.P == sc.P), MC_ERR_STATE,
                   "no scene points: pass scene_xyz or call mc_scene_set_points");
        sync_stats(ctx);
        hipStream_t s = ctx->stream;
        const int K = cl.K, N0 = gr.N0, FW = sc.FW, M = sc.M, Min = sc.M_in;
        const int64_t P = sc.P, np = ctx->h_stats[ST_NPTS];
        DevBuf scene, moff, mlen, cnt, keepf, nid, dnn, sel, plen, qlen, inidx, nvf, qcol;
        const double *d_scene = scene_xyz;
        {
            mc::TimedScope ts(ctx->timer, s, "pp_prep");
            if (!scene_xyz) {  // the float32 points, widened exactly
                scene.reserve(static_cast<size_t>(P) * 24 + 8);
                hipLaunchKernelGGL(mc::k_pp_widen, grid_for(3 * P), dim3(256), 0, s, ctx->bp.scene.as<float>(), 3 * P,
                                   scene.as<double>());
                d_scene = scene.as<double>();
            } else if (!scene_on_device) {
                scene.reserve(static_cast<size_t>(P) * 24 + 8);
                if (P) MC_HIP(hipMemcpyAsync(scene.ptr, scene_xyz, static_cast<size_t>(P) * 24, hipMemcpyHostToDevice, s));
                d_scene = scene.as<double>();
            }
            // the mask table in input order: rows of skipped frames (not in the context's table) are empty
            const int *d_inidx = nullptr;
            if (M != Min) {
                inidx.reserve(static_cast<size_t>(M) * 4 + 8);
                if (M) MC_HIP(hipMemcpyAsync(inidx.ptr, sc.h_in_index.data(), static_cast<size_t>(M) * 4, hipMemcpyHostToDevice, s));
                d_inidx = inidx.as<int>();
            }
            mlen.reserve(static_cast<size_t>(Min) * 4 + 8);
            moff.reserve(static_cast<size_t>(Min + 1) * 8);
            MC_HIP(hipMemsetAsync(mlen.ptr, 0, static_cast<size_t>(Min) * 4 + 4, s));
            if (M) hipLaunchKernelGGL(mc::k_pp_cl_masklen, grid_for(M), dim3(256), 0, s, M, d_inidx, sc.d_mask_off.as<int>(),
                                      mlen.as<int>());
            hipLaunchKernelGGL(mc::k_pp_scan64<int>, dim3(1), dim3(1024), 0, s, mlen.as<int>(), Min, moff.as<int64_t>());
            // nodes: the objects with at least 2 level-0 masks, in object order
            cnt.reserve(static_cast<size_t>(K) * 4 + 8);
            keepf.reserve(static_cast<size_t>(K) * 4 + 8);
            nid.reserve(static_cast<size_t>(K + 1) * 4 + 8);
            dnn.reserve(8);
            MC_HIP(hipMemsetAsync(cnt.ptr, 0, static_cast<size_t>(K) * 4 + 4, s));
            if (N0) hipLaunchKernelGGL(mc::k_pp_cl_count, grid_for(N0), dim3(256), 0, s, N0, cl.d_final_label.as<int>(),
                                       cnt.as<int>());
            if (K) hipLaunchKernelGGL(mc::k_pp_cl_keep, grid_for(K), dim3(256), 0, s, K, cnt.as<int>(), keepf.as<int>());
            mc::scan_device_n(s, keepf.as<int>(), nid.as<int>(), nullptr, K, dnn.as<int>());
            MC_HIP(hipGetLastError());
        }
        int Nn = 0;
        MC_HIP(hipMemcpyAsync(&Nn, dnn.ptr, 4, hipMemcpyDeviceToHost, s));
        MC_HIP(hipStreamSynchronize(s));
        MC_REQUIRE(Nn >= 0 && Nn <= K, MC_ERR_HIP, "node count out of range");
        sel.reserve(static_cast<size_t>(Nn) * 4 + 8);
        plen.reserve(static_cast<size_t>(Nn) * 4 + 8);
        qlen.reserve(static_cast<size_t>(Nn) * 4 + 8);
        nvf.reserve(static_cast<size_t>(Nn) * FW * 8 + 8);
        qcol.reserve(static_cast<size_t>(N0) * 4 + 8);
        pp.d_npoff.reserve(static_cast<size_t>(Nn + 1) * 8);
        pp.d_qoff.reserve(static_cast<size_t>(Nn + 1) * 8);
        pp.d_npts.reserve(static_cast<size_t>(np) * 4 + 8);
        pp.d_qm.reserve(static_cast<size_t>(N0) * 4 + 8);
        {
            mc::TimedScope ts(ctx->timer, s, "pp_prep");
            if (K) hipLaunchKernelGGL(mc::k_pp_cl_select, grid_for(K), dim3(256), 0, s, K, cnt.as<int>(), nid.as<int>(),
                                      cl.d_ptoff_out.as<int>(), sel.as<int>(), plen.as<int>(), qlen.as<int>());
            hipLaunchKernelGGL(mc::k_pp_scan64<int>, dim3(1), dim3(1024), 0, s, plen.as<int>(), Nn, pp.d_npoff.as<int64_t>());
            hipLaunchKernelGGL(mc::k_pp_scan64<int>, dim3(1), dim3(1024), 0, s, qlen.as<int>(), Nn, pp.d_qoff.as<int64_t>());
            if (Nn) {
                hipLaunchKernelGGL(mc::k_pp_cl_members, dim3(std::min(ceil_div(Nn, 4), 4096)), dim3(256), 0, s, Nn, N0,
                                   sel.as<int>(), cl.d_final_label.as<int>(), gr.d_node0_g.as<int>(),
                                   M != Min ? inidx.as<int>() : nullptr, sc.d_mask_col.as<int>(),
                                   pp.d_qoff.as<int64_t>(), pp.d_qm.as<int>(), qcol.as<int>());
                hipLaunchKernelGGL(mc::k_pp_cl_gather, dim3(std::min(Nn, 4096)), dim3(256), 0, s, Nn, FW, sel.as<int>(),
                                   cl.d_ptoff_out.as<int>(), cl.d_pts_out.as<int>(), cl.fin.vf,
                                   pp.d_npoff.as<int64_t>(), pp.d_npts.as<int>(), nvf.as<unsigned long long>());
            }
            MC_HIP(hipGetLastError());
        }
        PPRun r;
        mc::PPArgs &a = r.a;
        a.P = P, a.F = sc.F, a.Mt = Min, a.N = Nn;
        a.scene = d_scene;
        a.pfm = gr.d_pfm.as<unsigned long long>();
        a.nvf = nvf.as<unsigned long long>();
        a.mask_off = moff.as<int64_t>(), a.npoff = pp.d_npoff.as<int64_t>(), a.qoff = pp.d_qoff.as<int64_t>();
        a.mask_pts = sc.d_mask_pts.as<int>(), a.npts = pp.d_npts.as<int>(), a.qm = pp.d_qm.as<int>();
        a.qcol = qcol.as<int>();
        pp_check_args(ctx, params, r, false);
        pp_run(ctx, r, false);
        pp.d_qcol.swap(qcol);
    });
}

int mc_pp_export_info(mc_ctx *ctx, int32_t *num_final, int64_t *num_points, int64_t *num_masks)
{
    return guarded(ctx, [&] {
        PpState &pp = ctx->pp;
        MC_REQUIRE(pp.have, MC_ERR_STATE, "no post-processing result");
        const int nf = pp.info.num_final;
        if (num_final) *num_final = nf;
        if (num_points) *num_points = pp.opoff[nf];
        if (num_masks) *num_masks = pp.omoff[nf];
    });
}

int mc_pp_export(mc_ctx *ctx, int64_t *obj_pt_off, int32_t *obj_pts, int64_t *obj_mask_off, int32_t *obj_masks,
                 double *obj_mask_cov, int32_t *obj_repre, int32_t *obj_node, int on_device)
{
    return guarded(ctx, [&] {
        PpState &pp = ctx->pp;
        MC_REQUIRE(pp.have, MC_ERR_STATE, "no post-processing result");
        pp_build_export(ctx);
        hipStream_t s = ctx->stream;
        const int nf = pp.info.num_final;
        const int64_t np = pp.opoff[nf], nm = pp.omoff[nf];
        auto cp = [&](void *dst, const DevBuf &src, size_t bytes) {
            if (dst && bytes)
                MC_HIP(hipMemcpyAsync(dst, src.ptr, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
        };
        cp(obj_pt_off, pp.d_opoff, static_cast<size_t>(nf + 1) * 8);
        cp(obj_pts, pp.d_opts, static_cast<size_t>(np) * 4);
        cp(obj_mask_off, pp.d_omoff, static_cast<size_t>(nf + 1) * 8);
        cp(obj_masks, pp.d_omask, static_cast<size_t>(nm) * 4);
        cp(obj_mask_cov, pp.d_ocov, static_cast<size_t>(nm) * 8);
        cp(obj_repre, pp.d_repre, static_cast<size_t>(nf) * 20);
        cp(obj_node, pp.d_finnode, static_cast<size_t>(nf) * 4);
        MC_HIP(hipStreamSynchronize(s));
    });
}

int mc_pp_export_pred_masks(mc_ctx *ctx, uint8_t *out, int on_device)
{
    return guarded(ctx, [&] {
        PpState &pp = ctx->pp;
        MC_REQUIRE(pp.have, MC_ERR_STATE, "no post-processing result");
        pp_build_export(ctx);
        hipStream_t s = ctx->stream;
        const int nf = pp.info.num_final;
        const int64_t P = pp.P, E = pp.info.num_entries;
        const size_t bytes = static_cast<size_t>(P) * nf;
        if (!bytes) return;
        MC_REQUIRE(out, MC_ERR_INVALID, "null argument");
        DevBuf tmp;
        uint8_t *d = out;
        if (!on_device) {
            tmp.reserve(bytes);
            d = tmp.as<uint8_t>();
        }
        MC_HIP(hipMemsetAsync(d, 0, bytes, s));
        {
            mc::TimedScope ts(ctx->timer, s, "pp_export");
            hipLaunchKernelGGL(mc::k_pp_ex_pred, grid_for(E), dim3(256), 0, s, E, pp.d_npts.as<int>(),
                               pp.d_eobj.as<int>(), pp.d_fslot.as<int>(), nf, d);
            MC_HIP(hipGetLastError());
        }
        if (!on_device) MC_HIP(hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, s));
        MC_HIP(hipStreamSynchronize(s));
        ctx->timer.collect();
    });
}

int mc_pp_get_info(mc_ctx *ctx, mc_pp_info *info)
{
    return guarded(ctx, [&] {
        MC_REQUIRE(ctx->pp.have, MC_ERR_STATE, "no post-processing result");
        MC_REQUIRE(info, MC_ERR_INVALID, "null argument");
        *info = ctx->pp.info;
    });
}

int mc_pp_get_results(mc_ctx *ctx, int32_t *entry_object, int32_t *mask_object, double *mask_coverage,
                      uint8_t *object_state, int32_t *object_node, double *object_bbox)
{
    return guarded(ctx, [&] {
        PpState &pp = ctx->pp;
        MC_REQUIRE(pp.have, MC_ERR_STATE, "no post-processing result");
        if (entry_object || mask_object || mask_coverage) pp_fetch_host(ctx);
        auto cp = [](void *dst, const void *src, size_t bytes) {
            if (dst && bytes) std::memcpy(dst, src, bytes);
        };
        cp(entry_object, pp.entry_obj.data(), pp.entry_obj.size() * 4);
        cp(mask_object, pp.qobj.data(), pp.qobj.size() * 4);
        cp(mask_coverage, pp.qcov.data(), pp.qcov.size() * 8);
        cp(object_state, pp.state.data(), pp.state.size());
        cp(object_node, pp.obj_node.data(), pp.obj_node.size() * 4);
        cp(object_bbox, pp.box.data(), pp.box.size() * 8);
    });
}

}  // extern "C"
