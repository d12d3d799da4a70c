// mc_bp_denoise.inl — S1 back-projection, bp_launch_denoise: the kernels beside and after the LDS
// classes: the deferred points' k-NN ring search, the classes' statistics and survivors, and the
// global-memory kernel for slots beyond the largest class.
namespace mc {

// a slot's grid in global memory, as mc_bp_ring.hpp's ring_mark and ring_walk read it (kept records only)
struct BpRingGrid {
    const double4 *pt;
    const int *bs;
    unsigned nb;
    // (no bounds test: coordinates are >= -2 (the origin lies below every point) and far below
    // kBpCellMax; a negative one makes a key with its top bits set, which no record has)
    __device__ __forceinline__ unsigned bucket(int x, int y, int z) const { return mod_mul(bp_hash3(x, y, z), nb); }
    __device__ __forceinline__ int start(unsigned b) const { return bs[b]; }
    __device__ __forceinline__ double4 rec(int q) const { return pt[q]; }
    __device__ __forceinline__ unsigned long long key(const double4 &p) const
    {
        return static_cast<unsigned long long>(__double_as_longlong(p.w));
    }
    __device__ __forceinline__ unsigned long long cell_key(int x, int y, int z) const { return pack3(x, y, z) | kKeptBit; }
};
// a thread's cell and offsets (RingWhere's members), parked in LDS: component k at [k * 256 + thread].  The
// walk uses them once per cell it takes, not per record, and the kernel has no registers to spare beside the
// k-NN list (128 at four waves per SIMD); volatile, or the reads would be hoisted into registers again
struct BpRingWhere {
    const volatile __attribute__((address_space(3))) int *c;
    const volatile __attribute__((address_space(3))) double *o;
    __device__ __forceinline__ int x() const { return c[0]; }
    __device__ __forceinline__ int y() const { return c[256]; }
    __device__ __forceinline__ int z() const { return c[512]; }
    __device__ __forceinline__ double ox() const { return o[0]; }
    __device__ __forceinline__ double oy() const { return o[256]; }
    __device__ __forceinline__ double oz() const { return o[512]; }
};

// (a4) k-NN of the deferred points of every LDS-class slot of a batch (k_bp_denoise_lds's list pass
// could not serve them): a thread per queued point, over its slot's grid in global memory.  The 27
// cells around the point's, then the shell of 98 around those (R = 1, R = 2), each ring marked and
// walked by the lane on its own (mc_bp_ring.hpp): cells whose nearest face is no nearer than the
// lane's current k-th distance are skipped (a's offsets in its cell, gaps shrunk by 1e-9 ce so the
// bound stays below every point's computed distance), the bucket bounds of the others are read in
// groups, and only the cells whose bucket holds records are walked, in one loop per ring: a wave
// takes as many trips as its longest lane has record pairs, not a dependent bounds read per cell of
// the cube (most cells of a surface patch are empty).  A point the rings cannot settle (sparse)
// scans every kept point.
template <int WPE = 1>
__global__ __launch_bounds__(256, WPE) void k_bp_knn_ring(const int *__restrict__ dq_cnt, const int *__restrict__ dq,
                                                     const int *__restrict__ slot_pix, const int *__restrict__ slot_m,
                                                     BpDev pr, const double4 *__restrict__ grec,
                                                     const int *__restrict__ gbs, const int *__restrict__ gitem,
                                                     const double *__restrict__ slot_grid, double *__restrict__ gavg,
                                                     int *__restrict__ err)
{
    __shared__ int s_c[3 * 256];
    __shared__ double s_o[3 * 256];
    const int ne = *dq_cnt;
    const int lane = lane_id();
    // wave-uniform loop (a wave's 64 points together), so that the whole wave can take a sparse
    // point's whole-cloud scan (below)
    const int nwv = gridDim.x * (256 / 64);
    for (int f0 = ((blockIdx.x * 256 + threadIdx.x) >> 6) * 64; f0 < ne; f0 += nwv * 64) {
        const int f = f0 + lane;
        bool active = f < ne;
        const int s = active ? dq[f] : 0;
        const int base = active ? slot_pix[s] : 0;
        const double *gm = slot_grid + 8 * static_cast<size_t>(s);
        double mn[3] = {0.0, 0.0, 0.0};
        BpLdsGrid g;
        g.pt = grec + base;
        g.bs = gbs + 2 * static_cast<size_t>(base) + s;
        g.nb = 1u;
        int n = 0;
        if (active) {
#pragma unroll
            for (int c = 0; c < 3; c++) mn[c] = gm[c];
            g.nb = static_cast<unsigned>(gm[6]);
            n = static_cast<int>(gm[7]);
#pragma unroll
            for (int c = 0; c < 3; c++) g.cmax[c] = static_cast<int>(gm[3 + c]);
        }
        int q = 0, r = 0;
        if (active) {
            const int item = gitem[f];
            q = item & 0x3FFF;
            r = item >> 14;
            // an entry outside its slot (a broken hand-off from the class kernel) is reported, not followed
            if (q >= n || r < 0 || r >= slot_m[s]) {
                atomicOr(err, 1);
                active = false;
            }
        }
        double best[kBpKnnMax];
#pragma unroll
        for (int k = 0; k < kBpKnnMax; k++) best[k] = DBL_MAX;
        int found = 0;
        bool done = false;
        double4 a = make_double4(0.0, 0.0, 0.0, 0.0);
        int x = 0, y = 0, z = 0;
        const double ce = pr.ce, sl = 1e-9 * pr.ce;
        double ox = 0.0, oy = 0.0, oz = 0.0;
        if (active) {
            a = g.pt[q];
            unpack3(static_cast<unsigned long long>(__double_as_longlong(a.w)) & ~kKeptBit, x, y, z);
            ox = fmin(fmax(a.x - mn[0] - x * ce, 0.0), ce);
            oy = fmin(fmax(a.y - mn[1] - y * ce, 0.0), ce);
            oz = fmin(fmax(a.z - mn[2] - z * ce, 0.0), ce);
        }
        s_c[threadIdx.x] = x;
        s_c[256 + threadIdx.x] = y;
        s_c[512 + threadIdx.x] = z;
        s_o[threadIdx.x] = ox;
        s_o[256 + threadIdx.x] = oy;
        s_o[512 + threadIdx.x] = oz;
        const BpRingWhere wh{(const volatile __attribute__((address_space(3))) int *)(s_c + threadIdx.x),
                             (const volatile __attribute__((address_space(3))) double *)(s_o + threadIdx.x)};
        const BpRingGrid rg{g.pt, g.bs, g.nb};
#pragma unroll 1
        for (int ring = 0; ring < 2; ring++) {  // rolled: one copy of the walk (instruction cache)
            if (!active || done) continue;
            const RingMask m = ring_mark(rg, ring, wh, ce, sl, best[kBpKnnMax - 1]);
            ring_walk(
                rg, ring, m, wh, a.x, a.y, a.z, ce, sl, [&] { return best[kBpKnnMax - 1]; },
                [&](double d2, bool on) {
                    sorted_insert(best, on ? d2 : DBL_MAX);
                    found += on ? 1 : 0;
                });
            const double reach = static_cast<double>(ring + 1) * ce;
            done = found >= kBpKnnMax && best[kBpKnnMax - 1] < reach * reach * (1.0 - 1e-9);
        }
#ifdef MC_BP_RING_NOFB
        done = true;  // timing-only diagnostics build: no whole-cloud fallback (wrong results)
#endif
        // the rings' k smallest -> the mean distance (the k-NN list's registers free for the scan below)
        double sum = 0.0;
        if (active && done) {
            if constexpr (MC_DBG_CHECK) {  // the ring result against every kept record of the slot's grid
                double bf[kBpKnnMax];
                for (int k = 0; k < kBpKnnMax; k++) bf[k] = DBL_MAX;
                for (int q2 = 0; q2 < n; q2++) {
                    const double4 p = g.pt[q2];
                    if (!(static_cast<unsigned long long>(__double_as_longlong(p.w)) & kKeptBit)) continue;
                    const double ex = a.x - p.x, ey = a.y - p.y, ez = a.z - p.z;
                    sorted_insert(bf, ((ex * ex) + (ey * ey)) + (ez * ez));
                }
                if (bf[kBpKnnMax - 1] != best[kBpKnnMax - 1] && bp_dbg_fail(4)) {
                    printf("[bp dbg ring] slot=%d n=%d q=%d cell (%d,%d,%d) cmax (%d,%d,%d) nb=%u found=%d done=%d best19 %.17g brute19 %.17g\n",
                           s, n, q, x, y, z, g.cmax[0], g.cmax[1], g.cmax[2], g.nb, found, done ? 1 : 0, best[kBpKnnMax - 1],
                           bf[kBpKnnMax - 1]);
                    printf("   a (%.17g, %.17g, %.17g) mn (%.17g, %.17g, %.17g) ce %.17g o (%.17g, %.17g, %.17g)\n", a.x, a.y, a.z,
                           mn[0], mn[1], mn[2], ce, ox, oy, oz);
                    for (int q2 = 0; q2 < n; q2++) {  // the kept records nearer than the ring's k-th
                        const double4 p = g.pt[q2];
                        const unsigned long long kw = static_cast<unsigned long long>(__double_as_longlong(p.w));
                        if (!(kw & kKeptBit)) continue;
                        const double ex = a.x - p.x, ey = a.y - p.y, ez = a.z - p.z;
                        const double d2 = ((ex * ex) + (ey * ey)) + (ez * ez);
                        if (d2 >= best[kBpKnnMax - 1]) continue;
                        int px, py, pz;
                        unpack3(kw & ~kKeptBit, px, py, pz);
                        const unsigned b = mod_mul(bp_hash3(px, py, pz), g.nb);
                        printf("   rec %d cell (%d,%d,%d) d2 %.17g bucket %u [%d,%d) p (%.17g, %.17g, %.17g)\n", q2, px, py, pz, d2, b,
                               g.bs[b], g.bs[b + 1], p.x, p.y, p.z);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kBpKnnMax; k++) sum = sum + sqrt(best[k]);
        }
        // sparse points (the rings could not settle them): every kept point of the slot, the whole
        // wave scanning one such point's slot (a lane's k smallest over its stride, then the k
        // smallest of the wave by k rounds of a wave minimum): the same k smallest values, in the
        // same ascending order, as one thread's scan, without one lane's O(n) walk holding the wave
        unsigned long long need = __ballot(active && !done);
        while (need) {
            const int L = __ffsll(static_cast<long long>(need)) - 1;
            need &= need - 1ull;
            auto bcast_d = [&](double v) {
                const long long b = __double_as_longlong(v);
                const int lo = __builtin_amdgcn_readlane(static_cast<int>(b & 0xFFFFFFFFll), L);
                const int hi = __builtin_amdgcn_readlane(static_cast<int>(b >> 32), L);
                return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
            };
            const double ax = bcast_d(a.x), ay = bcast_d(a.y), az = bcast_d(a.z);
            const int nL = __builtin_amdgcn_readlane(n, L), baseL = __builtin_amdgcn_readlane(base, L);
            const double4 *ptL = grec + baseL;
            double bl[kBpKnnMax];
#pragma unroll
            for (int k = 0; k < kBpKnnMax; k++) bl[k] = DBL_MAX;
            for (int q2 = lane; q2 < nL; q2 += 64) {
                const double4 p = ptL[q2];
                if (!(static_cast<unsigned long long>(__double_as_longlong(p.w)) & kKeptBit)) continue;
                const double ex = ax - p.x, ey = ay - p.y, ez = az - p.z;
                sorted_insert(bl, ((ex * ex) + (ey * ey)) + (ez * ez));
            }
#pragma unroll
            for (int k = 0; k < kBpKnnMax; k++) {
                const double h = bl[0];
                const double m = wave_min_d(h);
                const unsigned long long w = __ballot(h == m);
                if (lane == __ffsll(static_cast<long long>(w)) - 1) {  // the lane holding it moves on
#pragma unroll
                    for (int j = 0; j + 1 < kBpKnnMax; j++) bl[j] = bl[j + 1];
                    bl[kBpKnnMax - 1] = DBL_MAX;
                }
                if (lane == L) sum = sum + sqrt(m);  // (k ascending, as the rings' sum above)
            }
        }
        if (active) {
            gavg[base + r] = sum / static_cast<double>(kBpKnnMax);
            bp_dbg_path(static_cast<size_t>(base) + r, 4u | (static_cast<unsigned>(found > 0xFFFF ? 0xFFFF : found) << 4) |
                                                         (static_cast<unsigned>(done ? 1 : 0) << 20));
        }
    }
}

// (a4) the end of denoise for every LDS-class slot (classes 0 .. kBpClasses-1), a wave per slot:
// remove_statistical_outlier's cloud mean and Bessel std of the m mean distances as sequential sums
// in index order (std::accumulate: 64 values read at once, then added in order as scalars), the
// survivors 0 < d < mean + std_ratio * std in index order -> float32 mask points and their AABB.
__global__ __launch_bounds__(256) void k_bp_denoise_tail(const int *__restrict__ cls_cnt, const int *__restrict__ cls_list,
                                                         int cap, int cls_lo, int cls_hi, const int *__restrict__ slot_pix,
                                                         const int *__restrict__ slot_m, BpDev pr,
                                                         const double *__restrict__ vpts, const double *__restrict__ gavg,
                                                         const int *__restrict__ gsx, float *__restrict__ qpts,
                                                         int *__restrict__ slot_ns, float *__restrict__ slot_box)
{
    int cnt[kBpClasses];
    int total = 0;
#pragma unroll
    for (int c = 0; c < kBpClasses; c++) {
        cnt[c] = c >= cls_lo && c < cls_hi ? cls_cnt[c] : 0;  // classes [cls_lo, cls_hi)
        total += cnt[c];
    }
    const int lane = lane_id();
    const int nwaves = gridDim.x * 4;
    for (int x = blockIdx.x * 4 + (threadIdx.x >> 6); x < total; x += nwaves) {
        int c = 0, o = x;
        while (o >= cnt[c]) o -= cnt[c++];
        const int s = cls_list[static_cast<size_t>(c) * cap + o];
        const int base = slot_pix[s], m = slot_m[s];
        const double *av = gavg + base;
        const double *P = vpts + 3 * static_cast<size_t>(base);
        if constexpr (MC_DBG_CHECK) bp_dbg_knn_tail(P, gsx + base, av, m, min(pr.knn, m), s, base);
        double mean = 0.0, sq = 0.0;
        // (each pass loads its next 64 values before the ordered chain of this 64 runs)
        double an = lane < m ? av[lane] : 0.0;
        for (int r0 = 0; r0 < m; r0 += 64) {
            // values that are not > 0 become +0.0, whose add leaves the (non-negative) sum as it is:
            // the ordered chain is plain adds, the selects run lane-parallel before it
            const double a = an;
            an = r0 + 64 + lane < m ? av[r0 + 64 + lane] : 0.0;
            mean = seq_add64_pos<false>(mean, a > 0 ? a : 0.0);
        }
        mean = mean / static_cast<double>(m);
        an = lane < m ? av[lane] : 0.0;
        for (int r0 = 0; r0 < m; r0 += 64) {
            const double v = an;
            an = r0 + 64 + lane < m ? av[r0 + 64 + lane] : 0.0;
            const double d = v > 0 ? (v - mean) * (v - mean) : 0.0;
            sq = seq_add64_pos<false>(sq, d > 0 ? d : 0.0);
        }
        const double sd = sqrt(sq / static_cast<double>(m - 1));
        const double thr = mean + pr.std_ratio * sd;
        int ns = 0;
        float flo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, fhi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        for (int r0 = 0; r0 < m; r0 += 64) {
            const int r = r0 + lane;
            const double v = r < m ? av[r] : 0.0;
            const bool keep = r < m && v > 0 && v < thr;
            const unsigned long long bal = __ballot(keep);
            if (keep) {
                const int i = gsx[base + r];
                float *qo = qpts + 3 * (static_cast<size_t>(base) + ns + __popcll(bal & ((1ull << lane) - 1ull)));
#pragma unroll
                for (int cc = 0; cc < 3; cc++) {
                    qo[cc] = static_cast<float>(P[3 * i + cc]);
                    flo[cc] = fminf(flo[cc], qo[cc]);
                    fhi[cc] = fmaxf(fhi[cc], qo[cc]);
                }
            }
            ns += __popcll(bal);
        }
#pragma unroll
        for (int cc = 0; cc < 3; cc++) {
            float a = flo[cc], b = fhi[cc];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                a = fminf(a, __shfl_xor(a, d, 64));
                b = fmaxf(b, __shfl_xor(b, d, 64));
            }
            if (lane == 0) {
                slot_box[6 * s + cc] = a;
                slot_box[6 * s + 3 + cc] = b;
            }
        }
        if (lane == 0) slot_ns[s] = ns;
    }
}

__global__ __launch_bounds__(256) void k_bp_denoise(
    const int *__restrict__ cls_cnt, const int *__restrict__ cls_list, const int *__restrict__ slot_pix, const int *__restrict__ slot_nv, BpDev pr,
    const double *__restrict__ vpts, unsigned long long *__restrict__ pcell, int *__restrict__ pbkt,
    int *__restrict__ bcnt, int *__restrict__ bstart, int *__restrict__ blist, int *__restrict__ ncnt,
    int *__restrict__ par, int *__restrict__ root, int *__restrict__ rnk, int *__restrict__ lab,
    int *__restrict__ ccnt, int *__restrict__ sidx, double *__restrict__ avg, float *__restrict__ qpts,
    int *__restrict__ slot_m, int *__restrict__ slot_ns, float *__restrict__ slot_box)
{
    __shared__ double red[24];
    __shared__ double s_avg[kBpStage];
    __shared__ int s_par[kBpLdsUF];
    __shared__ int s_nfb;
    __shared__ double s_thr;
    __shared__ float fred[24];
    __shared__ int ws[4];
    const int NL = *cls_cnt;
    const int t = threadIdx.x, lane = lane_id(), wv = t >> 6;
#ifdef MC_BP_STAMPS
    unsigned long long stamp_prev = __builtin_amdgcn_s_memrealtime();
#endif
    for (int k = blockIdx.x; k < NL; k += gridDim.x) {  // the slots of more than kBpLdsN voxels
        BP_STAMP(0);
        const int s = cls_list[k];
        const int base = slot_pix[s], n = slot_nv[s];
        const double *P = vpts + 3 * static_cast<size_t>(base);
        unsigned long long *pc = pcell + base;
        int *pb = pbkt + base, *bc = bcnt + 2 * static_cast<size_t>(base), *bs = bstart + 2 * static_cast<size_t>(base) + s;
        int *bl = blist + base, *nc = ncnt + base, *pa = par + base, *ro = root + base, *rk = rnk + base;
        int *lb = lab + base, *cc = ccnt + base + s, *si = sidx + base;
        double *av = avg + base;
        const unsigned nb = 2u * static_cast<unsigned>(n);
        // 1. bounding box -> grid origin and cell range
        double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, mx[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
        for (int i = t; i < n; i += 256)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                mn[c] = fmin(mn[c], P[3 * i + c]);
                mx[c] = fmax(mx[c], P[3 * i + c]);
            }
        block_minmax3(mn, mx, red);
        BpCells g;
        g.pc = pc;
        g.bs = bs;
        g.bl = bl;
        g.nb = nb;
#pragma unroll
        for (int c = 0; c < 3; c++) g.cmax[c] = static_cast<int>(floor((mx[c] - mn[c]) / pr.ce));
        BP_STAMP(1);
        // 2. cells, bucket counts; class counters cleared
        for (int i = t; i < n; i += 256) {
            int cxyz[3];
#pragma unroll
            for (int c = 0; c < 3; c++) cxyz[c] = static_cast<int>(floor((P[3 * i + c] - mn[c]) / pr.ce));
            pc[i] = pack3(cxyz[0], cxyz[1], cxyz[2]);
            const unsigned b = mod_mul(bp_hash3(cxyz[0], cxyz[1], cxyz[2]), nb);
            pb[i] = static_cast<int>(b);
            atomicAdd(&bc[b], 1);
        }
        for (int i = t; i <= n; i += 256) cc[i] = 0;
        sync_global();
        BP_STAMP(2);
        // 3. bucket starts
        {
            int carry = 0;
            for (int b0 = 0; b0 < static_cast<int>(nb); b0 += 256) {
                const int b = b0 + t;
                const int v = b < static_cast<int>(nb) ? ld_agent(&bc[b]) : 0;
                int tot;
                const int ex = block_excl_scan<256>(v, ws, tot);
                if (b < static_cast<int>(nb)) bs[b] = carry + ex;
                carry += tot;
            }
            if (t == 0) bs[nb] = carry;
        }
        sync_global();
        BP_STAMP(3);
        // 4. counting-sort scatter (bucket counters return to zero)
        for (int i = t; i < n; i += 256) {
            const int b = pb[i];
            bl[bs[b] + atomicSub(&bc[b], 1) - 1] = i;
        }
        sync_global();
        auto cell_of = [&](int i, int &x, int &y, int &z) {
            const unsigned long long k = pc[i];
            x = static_cast<int>(k >> 42);
            y = static_cast<int>((k >> 21) & 0x1FFFFF);
            z = static_cast<int>(k & 0x1FFFFF);
        };
        BP_STAMP(4);
        // 5. eps-neighbour counts (self included) -> core
        for (int i = t; i < n; i += 256) {
            int x, y, z;
            cell_of(i, x, y, z);
            int cnt = 0;
            const double *pi = P + 3 * i;
            for (int R = 0; R <= 1; R++)
                bp_shell(g, x, y, z, R, [&](int j) { cnt += bp_d2(pi, P + 3 * j) < pr.eps2 ? 1 : 0; });
            nc[i] = cnt;
            if (n <= kBpLdsUF) s_par[i] = i;
            else pa[i] = i;
        }
        sync_global();
        BP_STAMP(5);
        // 6. connected core points (union-find, root = smallest index)
        for (int i = t; i < n; i += 256) {
            if (nc[i] < pr.minpts) continue;
            int x, y, z;
            cell_of(i, x, y, z);
            const double *pi = P + 3 * i;
            for (int R = 0; R <= 1; R++)
                bp_shell(g, x, y, z, R, [&](int j) {
                    if (j < i && nc[j] >= pr.minpts && bp_d2(pi, P + 3 * j) < pr.eps2) {
                        if (n <= kBpLdsUF) uf_unite_s(s_par, i, j);
                        else uf_unite(pa, i, j);
                    }
                });
        }
        sync_global();
        BP_STAMP(6);
        // 7. clusters numbered in order of their smallest point
        {
            int carry = 0;
            for (int i0 = 0; i0 < n; i0 += 256) {
                const int i = i0 + t;
                int isr = 0;
                if (i < n && nc[i] >= pr.minpts) {
                    const int r = n <= kBpLdsUF ? uf_find_s(s_par, i) : uf_find(pa, i);
                    ro[i] = r;
                    isr = r == i ? 1 : 0;
                }
                int tot;
                const int ex = block_excl_scan<256>(isr, ws, tot);
                if (isr) rk[i] = carry + ex;
                carry += tot;
            }
        }
        sync_global();
        BP_STAMP(7);
        // 8. labels (+1 = the reference's shifted labels, geometry.py:10) and class counts
        for (int i = t; i < n; i += 256) {
            int l;
            if (nc[i] >= pr.minpts) {
                l = rk[ro[i]];
            } else {
                int x, y, z;
                cell_of(i, x, y, z);
                const double *pi = P + 3 * i;
                int mr = INT_MAX;
                for (int R = 0; R <= 1; R++)
                    bp_shell(g, x, y, z, R, [&](int j) {
                        if (nc[j] >= pr.minpts && bp_d2(pi, P + 3 * j) < pr.eps2) mr = min(mr, ro[j]);
                    });
                l = mr == INT_MAX ? -1 : rk[mr];
            }
            lb[i] = l;
            atomicAdd(&cc[l + 1], 1);
        }
        sync_global();
        BP_STAMP(8);
        // 9. class filter (geometry.py:15-20): the kept set S in index order
        const double lim = pr.frac * static_cast<double>(n);
        int m = 0;
        for (int i0 = 0; i0 < n; i0 += 256) {
            const int i = i0 + t;
            const int keep = (i < n && !(static_cast<double>(ld_agent(&cc[lb[i] + 1])) < lim)) ? 1 : 0;
            int tot;
            const int ex = block_excl_scan<256>(keep, ws, tot);
            if (keep) si[m + ex] = i;
            if (i < n) nc[i] = keep ? (nc[i] | (1 << 30)) : (nc[i] & ~(1 << 30));
            m += tot;
        }
        sync_global();
        BP_STAMP(9);
        // 10. k nearest kept points: grid rings up to R = 2, then (rare: sparse points) all of S
        const int kk = min(pr.knn, m);
        bp_knn<kBpKnnMax>(g, P, nc, si, m, kk, pr.ce, av, t, s_par, kBpLdsUF, &s_nfb);
        sync_global();
        BP_STAMP(10);
        // 11. cloud mean and Bessel std: sequential sums in index order (std::accumulate)
        {
            double mean = 0.0, sq = 0.0;
            for (int pass = 0; pass < 2; pass++) {
                for (int c0 = 0; c0 < m; c0 += kBpStage) {
                    const int cn = min(kBpStage, m - c0);
                    for (int x = t; x < cn; x += 256) s_avg[x] = av[c0 + x];
                    sync_global();
                    if (t == 0) {
                        for (int x = 0; x < cn; x++) {
                            const double a = s_avg[x];
                            if (pass == 0) {
                                if (a > 0) mean = mean + a;
                            } else {
                                sq = sq + (a > 0 ? (a - mean) * (a - mean) : 0.0);
                            }
                        }
                    }
                    sync_global();
                }
                if (pass == 0 && t == 0) mean = mean / static_cast<double>(m);
            }
            if (t == 0) {
                const double sd = sqrt(sq / static_cast<double>(m - 1));
                s_thr = mean + pr.std_ratio * sd;
            }
        }
        sync_global();
        const double thr = s_thr;
        BP_STAMP(11);
        // 12. survivors -> float32 mask points (:112) and their float32 AABB (:59-61)
        int ns = 0;
        float flo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, fhi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        for (int r0 = 0; r0 < m; r0 += 256) {
            const int r = r0 + t;
            const int keep = (r < m && av[r] > 0 && av[r] < thr) ? 1 : 0;
            int tot;
            const int ex = block_excl_scan<256>(keep, ws, tot);
            if (keep) {
                const int i = si[r];
                float *q = qpts + 3 * (static_cast<size_t>(base) + ns + ex);
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    q[c] = static_cast<float>(P[3 * i + c]);
                    flo[c] = fminf(flo[c], q[c]);
                    fhi[c] = fmaxf(fhi[c], q[c]);
                }
            }
            ns += tot;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float a = flo[c], b = fhi[c];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                a = fminf(a, __shfl_xor(a, d, 64));
                b = fmaxf(b, __shfl_xor(b, d, 64));
            }
            if (lane == 0) {
                fred[c * 4 + wv] = a;
                fred[12 + c * 4 + wv] = b;
            }
        }
        sync_global();
        BP_STAMP(12);
        if (t == 0) {
            slot_m[s] = m;
            slot_ns[s] = ns;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                slot_box[6 * s + c] = fminf(fminf(fred[c * 4], fred[c * 4 + 1]), fminf(fred[c * 4 + 2], fred[c * 4 + 3]));
                slot_box[6 * s + 3 + c] =
                    fmaxf(fmaxf(fred[12 + c * 4], fred[12 + c * 4 + 1]), fmaxf(fred[12 + c * 4 + 2], fred[12 + c * 4 + 3]));
            }
        }
        sync_global();
    }
}

}  // namespace mc
