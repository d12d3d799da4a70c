// mc_bp_query.inl — S1 back-projection, bp_launch_query: crop, ball query, coverage and neighbour set
// of every slot, staged in LDS (k_bp_query_lds) or walking the scene grid (k_bp_query).
namespace mc {

// ---------------------------------------------------------------------------------------------
// The rules k_bp_query and k_bp_query_lds share: each is bit-exact, so each has one definition
// ---------------------------------------------------------------------------------------------
// The cells [lo_c, hi_c] of one axis that the ball of a mask point at q can reach: a scene point with
// d2 < r^2 (float, bp_in_ball) has |dx|, |dy|, |dz| <= r, and the cells are 2r wide (inv = 1 / 2r), so
// the cells of [q - r, q + r] widened by a rounding margin (0.01 cell + the float error of q * inv):
// 2 per axis (8 cells) but where the margin crosses a cell border, instead of 27.
__device__ __forceinline__ void bp_reach_cells(float q, float inv, int &lo_c, int &hi_c)
{
    const float c = q * inv;
    const float m = 0.01f + fabsf(c) * 2e-6f;
    lo_c = min(max(static_cast<int>(floorf(c - 0.5f - m)), -kCellBias), kCellBias - 1) + kCellBias;
    hi_c = min(max(static_cast<int>(floorf(c + 0.5f + m)), -kCellBias), kCellBias - 1) + kCellBias;
}

// pytorch3d ball_query's test (u4) of scene point p against the mask point q: float, the CUDA kernel's
// one FMA chain written out
__device__ __forceinline__ bool bp_in_ball(float qx, float qy, float qz, const float4 &p, float r2)
{
    const float ex = qx - p.x, ey = qy - p.y, ez = qz - p.z;
    const float d2 = __fmaf_rn(ez, ez, __fmaf_rn(ey, ey, __fmul_rn(ex, ex)));
    return d2 < r2;
}

// the result of slot s when it has fewer than few_points mask points (:109): not kept, nothing queried
__device__ __forceinline__ void bp_slot_few(int s, int *__restrict__ slot_nn, int *__restrict__ slot_cov,
                                            int *__restrict__ slot_toff, int *__restrict__ kflag,
                                            int *__restrict__ ksize)
{
    slot_nn[s] = -1;
    slot_cov[s] = 0;
    slot_toff[s] = 0;
    kflag[s] = 0;
    ksize[s] = 0;
}

// the result of a queried slot s: covered of its mask points have an accepted neighbour; kept (:145), its
// set of n scene ids starts at tmp[b0]; kflag and ksize are the flags and sizes of the output scan
__device__ __forceinline__ void bp_slot_result(int s, bool kept, int n, int b0, int covered, int *__restrict__ slot_nn,
                                               int *__restrict__ slot_toff, int *__restrict__ slot_cov,
                                               int *__restrict__ kflag, int *__restrict__ ksize)
{
    slot_nn[s] = kept ? n : -1;
    slot_toff[s] = b0;
    slot_cov[s] = covered;
    kflag[s] = kept ? 1 : 0;
    ksize[s] = kept ? n : 0;
}

// ---------------------------------------------------------------------------------------------
// (a5-a7) crop + ball query + coverage + neighbour set, workgroup per slot (persistent grid)
// ---------------------------------------------------------------------------------------------
// For every float32 mask point q: the scene points of the 27 grid cells around q that lie strictly
// inside the mask's float32 AABB (crop_scene_points, :59-66) and have
// fmaf(dz, dz, fmaf(dy, dy, dx*dx)) < r^2 (pytorch3d ball_query, u4); the first K of them in scene
// index order (= crop order, :38,123-128) are accepted.  Accepted ids are OR'ed into the block's
// private bitmap over the scene; coverage = #q with an accepted neighbour / #q (:143); a kept mask
// (:145) emits its set in ascending order through a bump allocator into tmp.  It runs after
// k_bp_query_lds (below) on the slots that kernel listed (order, *dNS of them): the few whose box or
// crop exceeds its LDS.  Like it, it writes the slot's kept flag and set size for the output scan.
template <int WPE = 1, int KB = kBpBallMax>
__global__ __launch_bounds__(256, WPE) void k_bp_query(
    const int *__restrict__ dNS, const int *__restrict__ slot_pix, const int *__restrict__ slot_ns,
    const float *__restrict__ slot_box, const float *__restrict__ qpts, BpDev pr, const float4 *__restrict__ gpts,
    const int *__restrict__ gidx, const unsigned long long *__restrict__ gcell, const int *__restrict__ gstart,
    unsigned gnb, unsigned long long *__restrict__ bm, int PW, int *__restrict__ tmp, int tmp_cap,
    int *__restrict__ tmp_top, int *__restrict__ slot_nn, int *__restrict__ slot_toff, int *__restrict__ slot_cov,
    int *__restrict__ ovf, const int *__restrict__ order, int *__restrict__ kflag, int *__restrict__ ksize)
{
    __shared__ int s_lo, s_hi, s_cov, s_base;
    __shared__ int ws[4];
    const int NS = *dNS;
    const int t = threadIdx.x, lane = lane_id();
    unsigned long long *mb = bm + static_cast<size_t>(blockIdx.x) * PW;
#ifdef MC_BP_STAMPS
    unsigned long long stamp_prev = __builtin_amdgcn_s_memrealtime();
#endif
    for (int idx = blockIdx.x; idx < NS; idx += gridDim.x) {  // the list k_bp_query_lds left, in its order
        const int s = order[idx];
        const int ns = slot_ns[s];
        if (ns < pr.few) {  // :109 (uniform)
            if (t == 0) bp_slot_few(s, slot_nn, slot_cov, slot_toff, kflag, ksize);
            continue;
        }
        BP_STAMP(41);
        const int base = slot_pix[s];
        float lo[3], hi[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            lo[c] = slot_box[6 * s + c];
            hi[c] = slot_box[6 * s + 3 + c];
        }
        if (t == 0) {
            s_lo = INT_MAX;
            s_hi = -1;
            s_cov = 0;
        }
        __syncthreads();
        int wlo = INT_MAX, whi = -1, cov = 0;
        for (int r = t; r < ns; r += 256) {
            const float *q = qpts + 3 * (static_cast<size_t>(base) + r);
            const float qx = q[0], qy = q[1], qz = q[2];
            const int cx = scene_cell(qx, pr.scene_inv), cy = scene_cell(qy, pr.scene_inv),
                      cz = scene_cell(qz, pr.scene_inv);
            int best[KB];  // (KB = 20 when ball_k <= 20: 12 VGPRs fewer, a sixth wave per SIMD)
#pragma unroll
            for (int x = 0; x < KB; x++) best[x] = INT_MAX;
            // the cells the ball can reach (bp_reach_cells).  The next cell's bucket range is loaded
            // while this cell's points are scanned.
            int cl[3], cn[3];
            {
                const float qq[3] = {qx, qy, qz};
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    int lo_c, hi_c;
                    bp_reach_cells(qq[a], pr.scene_inv, lo_c, hi_c);
                    cl[a] = lo_c;
                    cn[a] = hi_c - lo_c + 1;
                }
            }
            (void)cx;
            (void)cy;
            (void)cz;
            const int ncell = cn[0] * cn[1] * cn[2];
            auto cell_range = [&](int d, unsigned long long &key) {
                const int x = cl[0] + d % cn[0], y = cl[1] + (d / cn[0]) % cn[1], z = cl[2] + d / (cn[0] * cn[1]);
                key = pack3(x, y, z);
                const unsigned b = mod_mul(bp_hash3(x, y, z), gnb);
                return make_int2(gstart[b], gstart[b + 1]);
            };
            unsigned long long nkey;
            int2 nrng = cell_range(0, nkey);
#pragma unroll 1
            for (int d = 0; d < ncell; d++) {
                const unsigned long long key = nkey;
                const int2 rng = nrng;
                if (d + 1 < ncell) nrng = cell_range(d + 1, nkey);
                // two records per step, each one's cell key and point + id (w) loaded together
                // (independent loads: one memory round trip per step instead of up to three dependent
                // ones); a step past the range re-reads its last record and ignores it
                auto take = [&](unsigned long long ck, const float4 &p) {
                    if (ck != key) return;
                    // (the crop's AABB test, inline: a function compiled differently; other copy: k_bp_query_lds 1.)
                    if (!(p.x > lo[0] && p.x < hi[0] && p.y > lo[1] && p.y < hi[1] && p.z > lo[2] && p.z < hi[2]))
                        return;
                    if (bp_in_ball(qx, qy, qz, p, pr.r2)) sorted_insert(best, __float_as_int(p.w));
                };
                for (int k = rng.x; k < rng.y; k += 2) {
                    const int k1 = min(k + 1, rng.y - 1);
                    const unsigned long long c0 = gcell[k], c1 = gcell[k1];
                    const float4 p0 = gpts[k], p1 = gpts[k1];
                    take(c0, p0);
                    if (k + 1 < rng.y) take(c1, p1);
                }
            }
            int got = 0;
#pragma unroll
            for (int x = 0; x < KB; x++) {
                if (x < pr.kball && best[x] != INT_MAX) {
                    const int id = best[x];
                    atomicOr(&mb[id >> 6], 1ull << (id & 63));
                    wlo = min(wlo, id >> 6);
                    whi = max(whi, id >> 6);
                    got = 1;
                }
            }
            cov += got;
        }
        wlo = wave_min_i(wlo);
        whi = wave_max_i(whi);
        cov = wave_sum(cov);
        if (lane == 0) {
            atomicMin(&s_lo, wlo);
            atomicMax(&s_hi, whi);
            atomicAdd(&s_cov, cov);
        }
        __syncthreads();
        BP_STAMP(42);
        const int covered = s_cov, wl = s_lo, wh = s_hi;
        const bool kept = !(static_cast<double>(covered) / static_cast<double>(ns) < pr.cov);
        const int RW = wh >= wl ? wh - wl + 1 : 0;
        const int per = (RW + 255) / 256;
        const int w0 = wl + t * per, w1 = min(wl + RW, w0 + per);
        int mine = 0;
        if (kept)
            for (int w = w0; w < w1; w++) mine += __popcll(__hip_atomic_load(&mb[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        int tot;
        int pos = block_excl_scan<256>(mine, ws, tot);
        if (t == 0) {
            int b0 = 0;
            if (kept) {
                b0 = atomicAdd(tmp_top, tot);
                if (b0 + tot > tmp_cap) atomicOr(ovf, 1);
            }
            s_base = b0;
            bp_slot_result(s, kept, tot, b0, covered, slot_nn, slot_toff, slot_cov, kflag, ksize);
        }
        __syncthreads();
        const int b0 = s_base;
        const bool room = kept && b0 + tot <= tmp_cap;
        for (int w = w0; w < w1; w++) {
            unsigned long long v = __hip_atomic_load(&mb[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            mb[w] = 0ull;  // the bitmap returns to zero
            if (!room) continue;
            while (v) {
                const int bt = __ffsll(static_cast<long long>(v)) - 1;
                v &= v - 1;
                tmp[b0 + pos++] = (w << 6) + bt;
            }
        }
        __syncthreads();
        BP_STAMP(43);
    }
}

// ---------------------------------------------------------------------------------------------
// (a5-a7) the same query with the slot's cropped scene points staged in LDS (the bulk of the slots)
// ---------------------------------------------------------------------------------------------
// A mask's points reach only the scene points strictly inside its float32 AABB, a few hundred, which
// k_bp_query fetches from the hashed grid once per mask point.  Here a workgroup enumerates the cells
// of the AABB once (mc_bp_qcell.hpp), a thread per cell and every bucket lookup independent, and puts
// the records that pass the key test and the AABB predicate into LDS, counting-sorted by box cell:
//   1. find    thread per box cell, four cells at a time (their bucket ranges, then their first records,
//              loaded together): the records of the cell inside the AABB are counted (s_cs[cell + 1]) and
//              their record index and cell appended to a staging list
//   2. scan    exclusive sums of the counts: s_cs[cell + 1] = the cell's start, s_cs[0] = 0
//   3. place   thread per staged record: (x, y, z, id) read again (independent loads) and written at its
//              cell's cursor, s_cs[cell + 1]++ (two u16 per atomic word), which leaves s_cs[c] = start of
//              cell c for c in [0, cells]
//   4. query   a thread per mask point: the reachable cells (k_bp_query's expression) clipped to the box,
//              one contiguous range of the sorted crop per (y, z) row; a counting pass that keeps the first
//              four hits, then (more hits) an accepting pass: the crop entries in the ball are flagged, all
//              of them when <= ball_k are in the ball, else the ball_k smallest scene ids, one per pass
//   5. emit    flagged ids compacted, ranked among themselves (their ascending order) and written to tmp
// The order of a cell's entries depends on the atomics' order; nothing else does (flags are per entry, the
// overfull selection goes by scene id, and the ids are distinct), so the outputs are deterministic.  A slot
// with more box cells than cell_cap or a larger crop than cand_cap is appended to fb_list for k_bp_query,
// as is every slot when cell_cap is 0.  Every per-slot LDS value is written before it is read within the
// slot (s_n, s_cov, s_cs [0, cells], the flags [0, crop)), and the slot body ends in a barrier on every
// path: no `continue` follows a single-lane action.
constexpr int kBpQcCells = 4096;  // box cells of a staged slot (98 % of the C3 masks cover fewer)
constexpr int kBpQcCand = 1024;   // cropped scene points of a staged slot
constexpr int kBpQcPer = kBpQcCells / 256;  // cells per thread of the scan
constexpr int kBpQcUnroll = 4;    // cells a thread looks up together
__global__ __launch_bounds__(256) void k_bp_query_lds(
    const int *__restrict__ dNS, const int *__restrict__ slot_pix, const int *__restrict__ slot_ns,
    const float *__restrict__ slot_box, const float *__restrict__ qpts, BpDev pr, const float4 *__restrict__ gpts,
    const unsigned long long *__restrict__ gcell, const int *__restrict__ gstart, unsigned gnb, int *__restrict__ tmp,
    int tmp_cap, int *__restrict__ tmp_top, int *__restrict__ slot_nn, int *__restrict__ slot_toff,
    int *__restrict__ slot_cov, int *__restrict__ ovf, const int *__restrict__ order, int *__restrict__ kflag,
    int *__restrict__ ksize, int *__restrict__ fb_list, int *__restrict__ fb_cnt, int cell_cap, int cand_cap)
{
    __shared__ float4 s_pt[kBpQcCand];                   // the crop, sorted by box cell: x, y, z, scene id
    __shared__ unsigned s_cw[(kBpQcCells + 8) / 2];      // s_cs, as the words of the cursors' atomics
    __shared__ __align__(16) int s_acc[kBpQcCand];       // staged record indices; then the accepted scene ids
    __shared__ unsigned short s_lc[kBpQcCand];           // staged records' cells; then s_flag
    __shared__ int s_n, s_cov, s_base;
    __shared__ int ws[4];
    unsigned short *const s_cs = reinterpret_cast<unsigned short *>(s_cw);  // per-cell counts, then starts
    unsigned char *const s_flag = reinterpret_cast<unsigned char *>(s_lc);  // crop entry accepted by some mask point
    const int NS = *dNS;
    const int t = threadIdx.x, lane = lane_id();
#ifdef MC_BP_STAMPS
    unsigned long long stamp_prev = __builtin_amdgcn_s_memrealtime();
#endif
    for (int idx = blockIdx.x; idx < NS; idx += gridDim.x) {  // largest slots first (k_bp_vox_order)
        const int s = order[idx];
        const int ns = slot_ns[s];
        const bool few = ns < pr.few;  // :109 (uniform, as every decision at slot level)
        float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
        QcBox bx = {{0, 0, 0}, {0, 0, 0}};
        int ncell = 0;
        bool staged = false;
        if (!few) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                lo[c] = slot_box[6 * s + c];
                hi[c] = slot_box[6 * s + 3 + c];
            }
            bx = qc_box(lo, hi, pr.scene_inv);
            const long long nc = qc_cells_capped(bx, cell_cap);
            staged = nc >= 1 && nc <= cell_cap;
            ncell = staged ? static_cast<int>(nc) : 0;
        }
        int ncand = 0;
        if (staged) {
            if (t == 0) {
                s_n = 0;
                s_cov = 0;
                s_cs[0] = 0;
            }
            __syncthreads();
            // 1. find
            for (int db = t; db < ncell; db += 256 * kBpQcUnroll) {
                unsigned long long key[kBpQcUnroll], c0[kBpQcUnroll];
                int k0[kBpQcUnroll], k1[kBpQcUnroll];
#pragma unroll
                for (int u = 0; u < kBpQcUnroll; u++) {
                    const int d = db + 256 * u;
                    key[u] = kEmptyKey;
                    k0[u] = k1[u] = 0;
                    if (d < ncell) {
                        int x, y, z;
                        qc_cell_of(d, bx, x, y, z);
                        key[u] = qc_key(x, y, z);
                        const unsigned b = mod_mul(bp_hash3(x, y, z), gnb);
                        k0[u] = gstart[b];
                        k1[u] = gstart[b + 1];
                    }
                }
#pragma unroll
                for (int u = 0; u < kBpQcUnroll; u++) c0[u] = k0[u] < k1[u] ? gcell[k0[u]] : kEmptyKey;
#pragma unroll
                for (int u = 0; u < kBpQcUnroll; u++) {
                    const int d = db + 256 * u;
                    int c = 0;
                    for (int k = k0[u]; k < k1[u]; k++) {
                        const unsigned long long ck = k == k0[u] ? c0[u] : gcell[k];
                        if (ck != key[u]) continue;
                        const float4 p = gpts[k];
                        // (the crop's AABB test; its other copy: k_bp_query's take)
                        if (!(p.x > lo[0] && p.x < hi[0] && p.y > lo[1] && p.y < hi[1] && p.z > lo[2] && p.z < hi[2]))
                            continue;
                        const int i = atomicAdd(&s_n, 1);
                        if (i < kBpQcCand) {
                            s_acc[i] = k;
                            s_lc[i] = static_cast<unsigned short>(qc_local(ck, bx));  // from the key the record carries
                        }
                        c++;
                    }
                    if (d < ncell) s_cs[d + 1] = static_cast<unsigned short>(min(c, 0xFFFF));
                }
            }
            __syncthreads();
            ncand = s_n;
            staged = ncand <= cand_cap;
        }
        BP_STAMP(44);
        if (staged) {
            // 2. scan (each thread reads and rewrites only its own cells' entries)
            {
                const int d0 = t * kBpQcPer;
                int c[kBpQcPer];
                int mine = 0;
#pragma unroll
                for (int j = 0; j < kBpQcPer; j++) {
                    c[j] = d0 + j < ncell ? s_cs[d0 + j + 1] : 0;
                    mine += c[j];
                }
                int tot;
                int pos = block_excl_scan<256>(mine, ws, tot);
#pragma unroll
                for (int j = 0; j < kBpQcPer; j++) {
                    if (d0 + j < ncell) s_cs[d0 + j + 1] = static_cast<unsigned short>(pos);
                    pos += c[j];
                }
            }
            __syncthreads();
            // 3. place
            for (int i = t; i < ncand; i += 256) {
                const float4 p = gpts[s_acc[i]];
                const unsigned w = static_cast<unsigned>(s_lc[i]) + 1u, sh = 16u * (w & 1u);
                const int at = static_cast<int>((atomicAdd(&s_cw[w >> 1], 1u << sh) >> sh) & 0xFFFFu);
                if (at < kBpQcCand) s_pt[at] = p;
            }
            __syncthreads();
            for (int i = t; i < ncand; i += 256) s_flag[i] = 0;  // (s_lc is read no more)
            __syncthreads();
            BP_STAMP(45);
            // 4. query
            const int base = slot_pix[s];
            const int nx = bx.n[0], nxy = bx.n[0] * bx.n[1];
            int cov = 0;
            for (int r = t; r < ns; r += 256) {
                const float *q = qpts + 3 * (static_cast<size_t>(base) + r);
                const float qx = q[0], qy = q[1], qz = q[2];
                // the cells the ball can reach (bp_reach_cells, rounding margin included), clipped to
                // the box and numbered within it
                int l0[3], l1[3];
                {
                    const float qq[3] = {qx, qy, qz};
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        int lo_c, hi_c;
                        bp_reach_cells(qq[a], pr.scene_inv, lo_c, hi_c);
                        l0[a] = max(lo_c - bx.o[a], 0);
                        l1[a] = min(hi_c - bx.o[a], bx.n[a] - 1);
                    }
                }
                auto in_ball = [&](const float4 &p) { return bp_in_ball(qx, qy, qz, p, pr.r2); };
                // every crop entry of the reachable cells: a contiguous range per (y, z) row
                auto walk = [&](auto &&f) {
                    if (l0[0] > l1[0]) return;
                    for (int z = l0[2]; z <= l1[2]; z++)
                        for (int y = l0[1]; y <= l1[1]; y++) {
                            const int row = z * nxy + y * nx;
                            const int k1 = s_cs[row + l1[0] + 1];
                            for (int k = s_cs[row + l0[0]]; k < k1; k++) f(k, s_pt[k]);
                        }
                };
                int cnt = 0;
                unsigned long long hits = 0ull;  // the first four entries in the ball, 16 bits each
                walk([&](int k, const float4 &p) {
                    if (!in_ball(p)) return;
                    if (cnt < 4) hits |= static_cast<unsigned long long>(k) << (16 * cnt);
                    cnt++;
                });
                if (cnt == 0) continue;
                cov++;
                if (cnt <= 4 && cnt <= pr.kball) {  // the usual case: no second pass
                    for (int j = 0; j < cnt; j++) s_flag[(hits >> (16 * j)) & 0xFFFFull] = 1;
                } else if (cnt <= pr.kball) {
                    walk([&](int k, const float4 &p) {
                        if (in_ball(p)) s_flag[k] = 1;
                    });
                } else {
                    // more than ball_k in the ball (rare): the ball_k smallest scene ids, one per pass
                    int last = -1;
                    for (int j = 0; j < pr.kball; j++) {
                        int best = INT_MAX, bk = -1;
                        walk([&](int k, const float4 &p) {
                            const int id = __float_as_int(p.w);
                            if (id > last && id < best && in_ball(p)) {
                                best = id;
                                bk = k;
                            }
                        });
                        if (bk >= 0) s_flag[bk] = 1;
                        last = best;
                    }
                }
            }
            cov = wave_sum(cov);
            if (lane == 0) atomicAdd(&s_cov, cov);
            __syncthreads();
            BP_STAMP(46);
            // 5. emit
            const int covered = s_cov;
            const bool kept = !(static_cast<double>(covered) / static_cast<double>(ns) < pr.cov);
            int na = 0;
            if (kept) {
                for (int i0 = 0; i0 < ncand; i0 += 256) {
                    const int i = i0 + t;
                    const int f = (i < ncand && s_flag[i]) ? 1 : 0;
                    int tot;
                    const int ex = block_excl_scan<256>(f, ws, tot);
                    if (f) s_acc[na + ex] = __float_as_int(s_pt[i].w);
                    na += tot;
                }
            }
            if (t == 0) {
                int b0 = 0;
                if (kept) {
                    b0 = atomicAdd(tmp_top, na);
                    if (b0 + na > tmp_cap) atomicOr(ovf, 1);
                }
                s_base = b0;
                bp_slot_result(s, kept, na, b0, covered, slot_nn, slot_toff, slot_cov, kflag, ksize);
            }
            __syncthreads();
            const int b0 = s_base;
            if (kept && b0 + na <= tmp_cap) {
                // scene ids are distinct: an id's rank among the accepted is its place in ascending order
                for (int i = t; i < na; i += 256) {
                    const int id = s_acc[i];
                    int rank = 0, j = 0;
                    for (; j + 4 <= na; j += 4) {  // the same address in every lane: one 16-byte LDS read
                        const int4 v = *reinterpret_cast<const int4 *>(&s_acc[j]);
                        rank += (v.x < id ? 1 : 0) + (v.y < id ? 1 : 0) + (v.z < id ? 1 : 0) + (v.w < id ? 1 : 0);
                    }
                    for (; j < na; j++) rank += s_acc[j] < id ? 1 : 0;
                    tmp[b0 + rank] = id;
                }
            }
        } else if (t == 0) {
            if (few) {
                bp_slot_few(s, slot_nn, slot_cov, slot_toff, kflag, ksize);
            } else {
                fb_list[atomicAdd(fb_cnt, 1)] = s;
            }
        }
        __syncthreads();
        BP_STAMP(47);
    }
}

}  // namespace mc
