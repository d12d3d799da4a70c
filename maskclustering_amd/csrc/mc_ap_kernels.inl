// mc_ap_kernels.inl — AP evaluation over accumulated scans on gfx950.
//
// evaluation/evaluate.py:254-329 (assign_instances_for_scan) on point lists and :53-205
// (evaluate_matches), restated in DESIGN.md §4:
//   k_ev_validate      range checks of one scan's inputs behind one flag word, and the largest id
//   k_ev_gt_count[_lds]  point count per ground-truth id (LDS histogram for id ranges up to kEvCountLds)
//   k_ev_gt_table      one workgroup: scan of the id range to the ascending distinct list, the class
//                      filter, the grouping by class (ids of one label are contiguous), id -> instance
//   k_ev_point_inst    per point: its instance index, -1 none, -2 void
//   k_ev_inter         workgroup per prediction: histogram of its points over the instances of its
//                      own class in LDS (kEvInstCap entries; a class with more instances is walked in
//                      windows of kEvInstCap, one pass over the point list per window), pairs emitted
//                      in ascending instance order
//   k_ev_pred_scan / k_ev_compact   numbering of the kept predictions, their tables and pair lists
//   k_ev_qual          per pair: the overlaps it passes (float64 division, compared with >)
//   k_ev_greedy        wave per (class, overlap) of one scan: the greedy pass over the ground truths
//   k_ev_fp            unmatched predictions -> false positives unless ignored
//   k_ev_cell_count / k_ev_cell_scan / k_ev_gather   examples of all scans, one segment per cell
//   k_ev_ap            workgroup per (class, overlap) cell: sort by score (LDS up to kEvSortCap
//                      examples, in place in global memory above), one precision/recall point per
//                      distinct score, step widths and the sum in index order
//   k_ev_run_count / k_ev_run_write   the accumulation as runs (mc_ev_state_export): workgroup per
//                      cell, the same sort (ev_block_sort), then per distinct key its true / false counts
//   k_ev_state_check   mc_ev_state_merge: the checks of a buffer's runs behind one flag word, and
//                      the 64-bit total of their examples
//   k_ev_state_scan / k_ev_state_expand / k_ev_state_units   the runs back to examples, thread per
//                      example, appended as one unit per non-empty cell
// No FMA is written (the library is built with -ffp-contract=off).

namespace mc {

constexpr int kEvInstCap = 512;     // instances of one class k_ev_inter counts in LDS at a time
constexpr int kEvSortCap = 2048;    // examples of one cell k_ev_ap sorts in LDS
constexpr int kEvMaxOverlaps = 32;  // one bit per overlap in k_ev_qual's masks
constexpr int kEvCountLds = 8192;   // ids k_ev_gt_count_lds counts in LDS

// exclusive scan of one int per thread over the workgroup (blockDim.x a multiple of 64, <= 1024)
// (restates block_excl_scan of mc_dev_common.inl for a block size known only at run time)
__device__ inline int ev_block_scan(int v, int *wsum /* LDS [17] */, int &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int x = v;
    for (int d = 1; d < 64; d <<= 1) {
        int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    __syncthreads();
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int i = 0; i < nw; i++) {
            int t = wsum[i];
            wsum[i] = s;
            s += t;
        }
        wsum[16] = s;
    }
    __syncthreads();
    total = wsum[16];
    return x - v + wsum[w];
}

__device__ __forceinline__ int ev_id(int g, int no_class, int base) { return no_class ? g % 1000 + base : g; }

// scores as sortable keys: ascending keys = ascending doubles, -0.0 == 0.0
__device__ __forceinline__ unsigned long long ev_key(double s)
{
    s += 0.0;
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(s));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ev_unkey(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double(static_cast<long long>(b));
}

// flag[0]: 1 negative ground-truth id, 2 point id out of [0, P), 4 offsets; flag[1]: largest id
__global__ __launch_bounds__(256) void k_ev_validate(int64_t P, const int *__restrict__ gt, int K,
                                                     const int64_t *__restrict__ off, int64_t npts,
                                                     const int *__restrict__ pts, int no_class, int base,
                                                     int *__restrict__ flag)
{
    const int64_t n = max(max(P, npts), static_cast<int64_t>(K) + 1);
    int bad = 0, mx = 0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
        if (i < P) {
            const int g = gt[i];
            if (g < 0) bad |= 1;
            else mx = max(mx, ev_id(g, no_class, base));
        }
        if (i < npts) {
            const int q = pts[i];
            if (q < 0 || q >= P) bad |= 2;
        }
        if (i <= K) {
            const int64_t o = off[i];
            if ((i == 0 && o != 0) || (i == K && o != npts) || o < 0 || o > npts) bad |= 4;
            if (i < K && off[i + 1] < o) bad |= 4;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        bad |= __shfl_xor(bad, d, 64);
        mx = max(mx, __shfl_xor(mx, d, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicOr(&flag[0], bad);
        atomicMax(&flag[1], mx);
    }
}

// Point count per id.  Ids below kEvCountLds (every --no_class scan: at most class_ids[0] * 1000 + 999)
// are counted in an LDS histogram per workgroup and flushed once; a larger id range goes to global
// atomics, one per distinct id of a wave's 64 points.
__global__ __launch_bounds__(256) void k_ev_gt_count_lds(int64_t P, const int *__restrict__ gt, int no_class, int base, int R,
                                                         int *__restrict__ cnt)
{
    __shared__ int h[kEvCountLds];
    for (int i = threadIdx.x; i < R; i += 256) h[i] = 0;
    __syncthreads();
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < P; i += static_cast<int64_t>(gridDim.x) * 256)
        atomicAdd(&h[ev_id(gt[i], no_class, base)], 1);
    __syncthreads();
    for (int i = threadIdx.x; i < R; i += 256)
        if (h[i]) atomicAdd(&cnt[i], h[i]);
}

__global__ __launch_bounds__(256) void k_ev_gt_count(int64_t P, const int *__restrict__ gt, int no_class, int base,
                                                     int *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
    for (int64_t i0 = static_cast<int64_t>(blockIdx.x) * 256 + (threadIdx.x & ~63); i0 < P; i0 += stride) {
        const bool valid = i0 + lane < P;
        const int id = valid ? ev_id(gt[i0 + lane], no_class, base) : -1;
        unsigned long long todo = __ballot(valid);
        while (todo) {
            const int l = __ffsll(static_cast<long long>(todo)) - 1;
            const int lid = __shfl(id, l, 64);
            const unsigned long long m = __ballot(valid && id == lid);
            if (lane == l) atomicAdd(&cnt[lid], __popcll(m));
            todo &= ~m;
        }
    }
}

__device__ __forceinline__ int ev_class_of(int label, const int *__restrict__ lab2cls, int nlab)
{
    return (label >= 0 && label < nlab) ? lab2cls[label] : -1;
}

// One workgroup of 1024.  class_cnt zeroed, class_first preset large, inst_of_id preset -1 by the host.
// info[0] = number of instances.
__global__ __launch_bounds__(1024) void k_ev_gt_table(int R, const int *__restrict__ cnt, const int *__restrict__ lab2cls,
                                                      int nlab, int C, int *__restrict__ tmp_id, int *__restrict__ class_cnt,
                                                      int *__restrict__ class_first, int *__restrict__ class_off,
                                                      int *__restrict__ gt_cls, int *__restrict__ gt_id,
                                                      int64_t *__restrict__ gt_vert, int *__restrict__ inst_of_id,
                                                      int *__restrict__ info)
{
    __shared__ int wsum[17];
    const int tid = threadIdx.x;
    const int ch = (R + 1023) / 1024;
    const int lo = min(R, tid * ch), hi = min(R, lo + ch);
    auto is_inst = [&](int id) { return id != 0 && cnt[id] > 0 && ev_class_of(id / 1000, lab2cls, nlab) >= 0; };
    int n = 0;
    for (int id = lo; id < hi; id++) n += is_inst(id) ? 1 : 0;
    int G;
    int at = ev_block_scan(n, wsum, G);
    for (int id = lo; id < hi; id++)
        if (is_inst(id)) tmp_id[at++] = id;
    __syncthreads();
    for (int i = tid; i < G; i += 1024) {
        const int c = lab2cls[tmp_id[i] / 1000];
        atomicAdd(&class_cnt[c], 1);
        atomicMin(&class_first[c], i);
    }
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int c = 0; c < C; c++) {
            class_off[c] = s;
            s += class_cnt[c];
        }
        class_off[C] = s;
        info[0] = G;
    }
    __syncthreads();
    for (int i = tid; i < G; i += 1024) {
        const int id = tmp_id[i], c = lab2cls[id / 1000];
        const int pos = class_off[c] + (i - class_first[c]);  // a label's ids are contiguous in the ascending list
        gt_cls[pos] = c;
        gt_id[pos] = id;
        gt_vert[pos] = cnt[id];
        inst_of_id[id] = pos;
    }
}

__global__ __launch_bounds__(256) void k_ev_point_inst(int64_t P, const int *__restrict__ gt, int no_class, int base,
                                                       const int *__restrict__ lab2cls, int nlab,
                                                       const int *__restrict__ inst_of_id, int *__restrict__ pinst)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < P; i += static_cast<int64_t>(gridDim.x) * 256) {
        const int id = ev_id(gt[i], no_class, base);
        pinst[i] = ev_class_of(id / 1000, lab2cls, nlab) < 0 ? -2 : inst_of_id[id];
    }
}

// Workgroup per prediction.  Pairs of prediction k go to pair_gt / pair_int[off[k] ..): a prediction
// of n points has at most n pairs.
__global__ __launch_bounds__(256) void k_ev_inter(int K, const int64_t *__restrict__ off, const int *__restrict__ pts,
                                                  const int *__restrict__ pcls_in, int no_class,
                                                  const int *__restrict__ lab2cls, int nlab, int min_region,
                                                  const int *__restrict__ pinst, const int *__restrict__ class_off,
                                                  int *__restrict__ keep, int *__restrict__ pcls, int64_t *__restrict__ pvert,
                                                  int64_t *__restrict__ pvoid, int *__restrict__ npair,
                                                  int *__restrict__ pair_gt, int64_t *__restrict__ pair_int)
{
    __shared__ int tab[kEvInstCap];
    __shared__ int s_void, wsum[17];
    const int tid = threadIdx.x;
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        const int64_t b = off[k], e = off[k + 1];
        const int c = no_class ? 0 : ev_class_of(pcls_in ? pcls_in[k] : 0, lab2cls, nlab);
        if (c < 0 || e - b < min_region) {
            if (tid == 0) {
                keep[k] = 0;
                npair[k] = 0;
            }
            continue;
        }
        const int g0 = class_off[c], ng = class_off[c + 1] - g0;
        int np = 0;
        int w0 = 0;
        do {
            const int wn = min(kEvInstCap, ng - w0);
            __syncthreads();
            for (int i = tid; i < wn; i += 256) tab[i] = 0;
            if (tid == 0 && w0 == 0) s_void = 0;
            __syncthreads();
            const int glo = g0 + w0;
            for (int64_t i = b + tid; i < e; i += 256) {
                const int q = pinst[pts[i]];
                if (q == -2) {
                    if (w0 == 0) atomicAdd(&s_void, 1);
                } else if (q >= glo && q < glo + wn) {
                    atomicAdd(&tab[q - glo], 1);
                }
            }
            __syncthreads();
            const int ch = (wn + 255) / 256;
            const int lo = min(wn, tid * ch), hi = min(wn, lo + ch);
            int n = 0;
            for (int i = lo; i < hi; i++) n += tab[i] != 0;
            int tot;
            int at = ev_block_scan(n, wsum, tot);
            for (int i = lo; i < hi; i++)
                if (tab[i] != 0) {
                    pair_gt[b + np + at] = glo + i;
                    pair_int[b + np + at] = tab[i];
                    at++;
                }
            np += tot;
            w0 += kEvInstCap;
        } while (w0 < ng);
        if (tid == 0) {
            keep[k] = 1;
            pcls[k] = c;
            pvert[k] = e - b;
            pvoid[k] = s_void;
            npair[k] = np;
        }
        __syncthreads();
    }
}

// One workgroup of 1024: kept[k] = number of kept predictions before k, pbase[k] = pairs before k;
// info[1] = kept predictions, info[2] = pairs.
__global__ __launch_bounds__(1024) void k_ev_pred_scan(int K, const int *__restrict__ keep, const int *__restrict__ npair,
                                                       int *__restrict__ kept, int *__restrict__ pbase, int *__restrict__ info)
{
    __shared__ int wsum[17];
    const int tid = threadIdx.x;
    const int ch = (K + 1023) / 1024;
    const int lo = min(K, tid * ch), hi = min(K, lo + ch);
    int nk = 0, np = 0;
    for (int k = lo; k < hi; k++) {
        nk += keep[k];
        np += npair[k];
    }
    int tk, tp;
    int ak = ev_block_scan(nk, wsum, tk);
    int ap = ev_block_scan(np, wsum, tp);
    for (int k = lo; k < hi; k++) {
        kept[k] = ak;
        pbase[k] = ap;
        ak += keep[k];
        ap += npair[k];
    }
    if (tid == 0) {
        info[1] = tk;
        info[2] = tp;
    }
}

// The scan's compact tables as one run of 8-byte words, laid out from info (instances, kept
// predictions, pairs): gt class / id / vert, prediction class / vert / void / score, pair
// prediction / ground truth / intersection.
__global__ __launch_bounds__(256) void k_ev_compact(int K, const int64_t *__restrict__ off, const int *__restrict__ keep,
                                                    const int *__restrict__ kept, const int *__restrict__ pbase,
                                                    const int *__restrict__ npair, const int *__restrict__ pcls,
                                                    const int64_t *__restrict__ pvert, const int64_t *__restrict__ pvoid,
                                                    const double *__restrict__ score_in, const int *__restrict__ pair_gt,
                                                    const int64_t *__restrict__ pair_int, const int *__restrict__ gt_cls,
                                                    const int *__restrict__ gt_id, const int64_t *__restrict__ gt_vert,
                                                    const int *__restrict__ info, int64_t *__restrict__ out)
{
    const int64_t G = info[0], Kk = info[1], NP = info[2];
    int64_t *o_gcls = out, *o_gid = out + G, *o_gvert = out + 2 * G;
    int64_t *o_cls = out + 3 * G, *o_vert = o_cls + Kk, *o_void = o_vert + Kk;
    double *o_score = reinterpret_cast<double *>(o_void + Kk);
    int64_t *o_ppred = o_void + 2 * Kk, *o_pgt = o_ppred + NP, *o_pint = o_pgt + NP;
    for (int64_t g = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; g < G; g += static_cast<int64_t>(gridDim.x) * 256) {
        o_gcls[g] = gt_cls[g];
        o_gid[g] = gt_id[g];
        o_gvert[g] = gt_vert[g];
    }
    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        if (!keep[k]) continue;
        const int j = kept[k], pb = pbase[k], n = npair[k];
        const int64_t b = off[k];
        if (threadIdx.x == 0) {
            o_cls[j] = pcls[k];
            o_vert[j] = pvert[k];
            o_void[j] = pvoid[k];
            o_score[j] = score_in ? score_in[k] : 1.0;
        }
        for (int i = threadIdx.x; i < n; i += 256) {
            o_ppred[pb + i] = j;
            o_pgt[pb + i] = pair_gt[b + i];
            o_pint[pb + i] = pair_int[b + i];
        }
    }
}

// ---- the greedy pass of one scan ---------------------------------------------------------------
// The scan's tables as 8-byte words (built by the host from the compact tables): per instance
// vert / id, per prediction vert / void / score / class slot, the pairs in ground-truth order
// (ascending prediction within an instance), per class slot its pair range, counts and example
// region.  The order of the words has one definition, ev_words() of mc_ap_plan.hpp.
struct EvScanDev {
    int G, K, NP, A, O;
    int64_t min_region;
    const int64_t *gvert, *gid;
    const int64_t *pvert, *pvoid, *pslot;
    const double *pscore;
    const int64_t *q_gt, *q_pred, *q_int;
    const int64_t *s_p0, *s_p1, *s_nfilt, *s_npred, *s_cls, *s_exoff, *s_cap;
    const double *overlaps;
    unsigned *qmask;        // [NP] per pair, ground-truth side (0 for filtered-out instances)
    unsigned *found;        // [K] overlaps at which a prediction has some instance, zeroed
    unsigned long long *ign;  // [K] ignored points besides the void ones, zeroed
    unsigned char *visited;   // [O * K], zeroed
    int64_t ex_base;        // this scan's region in the example arrays
    int unit_base;
    unsigned long long *ex_key;
    unsigned char *ex_true;
    int *unit_cell, *unit_cnt;
    int64_t *unit_off;
    unsigned long long *cell_hardfn;
    unsigned *cell_flags;
};

__global__ __launch_bounds__(256) void k_ev_qual(EvScanDev d)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < d.NP; i += gridDim.x * 256) {
        const int g = static_cast<int>(d.q_gt[i]), p = static_cast<int>(d.q_pred[i]);
        const int64_t I = d.q_int[i], gv = d.gvert[g];
        const double ov = static_cast<double>(I) / static_cast<double>(gv + d.pvert[p] - I);
        unsigned m = 0;
        for (int o = 0; o < d.O; o++) m |= (ov > d.overlaps[o]) ? (1u << o) : 0u;
        const bool group = d.gid[g] < 1000, small = gv < d.min_region;
        d.qmask[i] = (group || small) ? 0u : m;
        if (m) atomicOr(&d.found[p], m);
        const unsigned long long add = (group ? I : 0) + (small ? I : 0);
        if (add) atomicAdd(&d.ign[p], add);
    }
}

// Wave per (class slot, overlap).  Every lane runs the serial part with the same values; lane 0 writes.
__global__ __launch_bounds__(256) void k_ev_greedy(EvScanDev d)
{
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= d.A * d.O) return;
    const int a = u / d.O, o = u % d.O;
    const int64_t p0 = d.s_p0[a], p1 = d.s_p1[a];
    const int64_t ex = d.ex_base + d.s_exoff[a] + o * d.s_cap[a];
    unsigned char *vis = d.visited + static_cast<int64_t>(o) * d.K;
    int n = 0, nmatched = 0, cur_g = -1;
    bool matched = false;
    double score = 0.0;
    auto emit = [&](double s, int t) {
        if (lane == 0) {
            d.ex_key[ex + n] = ev_key(s);
            d.ex_true[ex + n] = static_cast<unsigned char>(t);
        }
        n++;
    };
    for (int64_t base = p0; base < p1; base += 64) {
        const int64_t i = base + lane;
        const bool q = i < p1 && ((d.qmask[i] >> o) & 1u);
        unsigned long long mask = __ballot(q);
        while (mask) {
            const int j = __ffsll(static_cast<long long>(mask)) - 1;
            mask &= mask - 1;
            const int g = static_cast<int>(d.q_gt[base + j]), p = static_cast<int>(d.q_pred[base + j]);
            if (g != cur_g) {
                if (matched) {
                    emit(score, 1);
                    nmatched++;
                }
                cur_g = g;
                matched = false;
            }
            if (vis[p]) continue;
            const double conf = d.pscore[p];
            if (matched) {  // the lower score is a false positive; p is not marked visited
                emit(conf < score ? conf : score, 0);
                score = conf > score ? conf : score;
            } else {
                matched = true;
                score = conf;
                vis[p] = 1;  // every lane stores the same byte and later reads its own store
            }
        }
    }
    if (matched) {
        emit(score, 1);
        nmatched++;
    }
    if (lane == 0) {
        const int cell = static_cast<int>(d.s_cls[a]) * d.O + o;
        d.unit_cell[d.unit_base + u] = cell;
        d.unit_off[d.unit_base + u] = ex;
        d.unit_cnt[d.unit_base + u] = n;
        const int64_t hf = d.s_nfilt[a] - nmatched;
        if (hf) atomicAdd(&d.cell_hardfn[cell], static_cast<unsigned long long>(hf));
        const unsigned f = (d.s_nfilt[a] > 0 ? 1u : 0u) | (d.s_npred[a] > 0 ? 2u : 0u);
        if (f) atomicOr(&d.cell_flags[cell], f);
    }
}

// after k_ev_greedy: thread per (prediction, overlap)
__global__ __launch_bounds__(256) void k_ev_fp(EvScanDev d)
{
    const int n = d.K * d.O;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256) {
        const int p = t / d.O, o = t % d.O;
        if ((d.found[p] >> o) & 1u) continue;
        const int64_t ign = d.pvoid[p] + static_cast<int64_t>(d.ign[p]);
        const double share = static_cast<double>(ign) / static_cast<double>(d.pvert[p]);
        if (!(share <= d.overlaps[o])) continue;
        const int a = static_cast<int>(d.pslot[p]);
        const int u = d.unit_base + a * d.O + o;
        const int64_t at = d.ex_base + d.s_exoff[a] + o * d.s_cap[a] + atomicAdd(&d.unit_cnt[u], 1);
        d.ex_key[at] = ev_key(d.pscore[p]);
        d.ex_true[at] = 0;
    }
}

// ---- the table over everything accumulated -----------------------------------------------------
__global__ __launch_bounds__(256) void k_ev_cell_count(int U, const int *__restrict__ unit_cell,
                                                       const int *__restrict__ unit_cnt, int *__restrict__ cell_n)
{
    for (int u = blockIdx.x * 256 + threadIdx.x; u < U; u += gridDim.x * 256)
        if (unit_cnt[u]) atomicAdd(&cell_n[unit_cell[u]], unit_cnt[u]);
}

// one workgroup of 1024: cell_off[NC + 1] from cell_n
__global__ __launch_bounds__(1024) void k_ev_cell_scan(int NC, const int *__restrict__ cell_n, int *__restrict__ cell_off)
{
    __shared__ int wsum[17];
    const int ch = (NC + 1023) / 1024;
    const int lo = min(NC, static_cast<int>(threadIdx.x) * ch), hi = min(NC, lo + ch);
    int n = 0;
    for (int i = lo; i < hi; i++) n += cell_n[i];
    int tot;
    int at = ev_block_scan(n, wsum, tot);
    for (int i = lo; i < hi; i++) {
        cell_off[i] = at;
        at += cell_n[i];
    }
    if (threadIdx.x == 0) cell_off[NC] = tot;
}

// workgroup per unit: its examples into its cell's segment (any order within a cell)
__global__ __launch_bounds__(256) void k_ev_gather(int U, const int *__restrict__ unit_cell, const int *__restrict__ unit_cnt,
                                                   const int64_t *__restrict__ unit_off, const int *__restrict__ cell_off,
                                                   int *__restrict__ cell_fill, const unsigned long long *__restrict__ ex_key,
                                                   const unsigned char *__restrict__ ex_true,
                                                   unsigned long long *__restrict__ key, unsigned char *__restrict__ tru)
{
    __shared__ int s_at;
    for (int u = blockIdx.x; u < U; u += gridDim.x) {
        const int n = unit_cnt[u];
        if (!n) continue;
        const int c = unit_cell[u];
        __syncthreads();
        if (threadIdx.x == 0) s_at = cell_off[c] + atomicAdd(&cell_fill[c], n);
        __syncthreads();
        const int at = s_at;
        const int64_t src = unit_off[u];
        for (int i = threadIdx.x; i < n; i += 256) {
            key[at + i] = ex_key[src + i];
            tru[at + i] = ex_true[src + i];
        }
    }
}

// Bitonic network with every exchange ascending, by the whole workgroup of 256 over K / T [0, n) in LDS
// or global memory: positions >= n act as +inf and never move.  The order within equal keys is free.
__device__ inline void ev_block_sort(unsigned long long *K, unsigned char *T, int n)
{
    const int tid = threadIdx.x;
    auto cmpx = [&](int i, int l) {
        if (l > i && l < n && K[l] < K[i]) {
            const unsigned long long tk = K[i];
            K[i] = K[l];
            K[l] = tk;
            const unsigned char tt = T[i];
            T[i] = T[l];
            T[l] = tt;
        }
    };
    for (int64_t k = 2; (k >> 1) < n; k <<= 1) {
        for (int i = tid; i < n; i += 256) cmpx(i, static_cast<int>(i ^ (k - 1)));
        __syncthreads();
        for (int64_t j = k >> 2; j > 0; j >>= 1) {
            for (int i = tid; i < n; i += 256) cmpx(i, static_cast<int>(i ^ j));
            __syncthreads();
        }
    }
}

// Workgroup per cell.  prec / rec: workspace of (examples + cells) doubles, cell c's at cell_off[c] + c.
// curve_cell >= 0: that cell's distinct scores and (tp, fp, fn) go to cv_*.
__global__ __launch_bounds__(256) void k_ev_ap(int NC, const int *__restrict__ cell_off, unsigned long long *__restrict__ key,
                                               unsigned char *__restrict__ tru, const unsigned long long *__restrict__ hardfn,
                                               const unsigned *__restrict__ flags, double *__restrict__ prec,
                                               double *__restrict__ rec, double *__restrict__ ap, int64_t *__restrict__ stats,
                                               int *__restrict__ ndist, int curve_cell, double *__restrict__ cv_score,
                                               int64_t *__restrict__ cv_tp, int64_t *__restrict__ cv_fp,
                                               int64_t *__restrict__ cv_fn)
{
    __shared__ unsigned long long lk[kEvSortCap];
    __shared__ unsigned char lt[kEvSortCap];
    __shared__ int wsum[17];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < NC; c += gridDim.x) {
        const int b = cell_off[c], n = cell_off[c + 1] - b;
        const unsigned f = flags[c];
        const int64_t hf = static_cast<int64_t>(hardfn[c]);
        unsigned long long *K = key + b;
        unsigned char *T = tru + b;
        __syncthreads();
        if (n <= kEvSortCap) {
            for (int i = tid; i < n; i += 256) {
                lk[i] = K[i];
                lt[i] = T[i];
            }
            K = lk;
            T = lt;
        }
        __syncthreads();
        ev_block_sort(K, T, n);
        int nt = 0;
        for (int i = tid; i < n; i += 256) nt += T[i];
        int ntrue;
        ev_block_scan(nt, wsum, ntrue);
        double *pr = prec + b + c, *rc = rec + b + c;
        int below = 0, nd = 0;  // true examples / distinct scores before the tile
        for (int t0 = 0; t0 < n; t0 += 256) {
            const int i = t0 + tid;
            const bool in = i < n;
            const int tv = in ? T[i] : 0;
            const int first = in && (i == 0 || K[i] != K[i - 1]);
            int tt, tf;
            const int bt = ev_block_scan(tv, wsum, tt) + below;
            const int j = ev_block_scan(first, wsum, tf) + nd;
            if (first) {
                const int64_t tp = ntrue - bt, fp = (n - i) - tp, fn = bt + hf;
                pr[j] = static_cast<double>(tp) / static_cast<double>(tp + fp);
                rc[j] = static_cast<double>(tp) / static_cast<double>(tp + fn);
                if (c == curve_cell) {
                    cv_score[j] = ev_unkey(K[i]);
                    cv_tp[j] = tp;
                    cv_fp[j] = fp;
                    cv_fn[j] = fn;
                }
            }
            below += tt;
            nd += tf;
        }
        __syncthreads();
        if (tid == 0) {
            double r = nan("");
            if ((f & 1u) && (f & 2u) && n > 0) {
                pr[nd] = 1.0;  // the artificial first point of the curve
                rc[nd] = 0.0;
                const int m = nd + 1;
                double acc = 0.0;
                for (int i = 0; i < m; i++) {
                    const double lo = rc[i == 0 ? 0 : i - 1], hi = (i + 1 < m) ? rc[i + 1] : 0.0;
                    const double w = 0.5 * lo - 0.5 * hi;
                    acc = acc + pr[i] * w;
                }
                r = acc;
            } else if (f & 1u) {
                r = 0.0;
            }
            ap[c] = r;
            stats[4 * c + 0] = n;
            stats[4 * c + 1] = ntrue;
            stats[4 * c + 2] = hf;
            stats[4 * c + 3] = f;
            ndist[c] = nd;
        }
    }
}

// ---- the accumulation as runs (mc_ev_state_*) ---------------------------------------------------
// A cell's examples as its distinct keys ascending, each with its count of true and false examples:
// the form AP depends on (include/mcgraph.h, the state buffer).

// Workgroup per cell, pass 1: the gathered segment sorted by key (left sorted in global memory) and
// the number of its distinct keys.
__global__ __launch_bounds__(256) void k_ev_run_count(int NC, const int *__restrict__ cell_off, unsigned long long *key,
                                                      unsigned char *tru, int *__restrict__ cell_nrun)
{
    __shared__ unsigned long long lk[kEvSortCap];
    __shared__ unsigned char lt[kEvSortCap];
    __shared__ int wsum[17];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < NC; c += gridDim.x) {
        const int b = cell_off[c], n = cell_off[c + 1] - b;
        unsigned long long *K = key + b;
        unsigned char *T = tru + b;
        const bool lds = n <= kEvSortCap;
        __syncthreads();
        if (lds) {
            for (int i = tid; i < n; i += 256) {
                lk[i] = K[i];
                lt[i] = T[i];
            }
            K = lk;
            T = lt;
        }
        __syncthreads();
        ev_block_sort(K, T, n);
        int nd = 0;
        for (int i = tid; i < n; i += 256) nd += (i == 0 || K[i] != K[i - 1]) ? 1 : 0;
        int tot;
        ev_block_scan(nd, wsum, tot);
        if (tid == 0) cell_nrun[c] = tot;
        if (lds)
            for (int i = tid; i < n; i += 256) {
                key[b + i] = lk[i];
                tru[b + i] = lt[i];
            }
    }
}

// Workgroup per cell, pass 2, over the sorted segments: run j of the cell at run_off[c] + j.  The
// first example of a run stores the counts of true / false examples below it; the differences of
// neighbours are the run's own counts.
__global__ __launch_bounds__(256) void k_ev_run_write(int NC, const int *__restrict__ cell_off,
                                                      const unsigned long long *__restrict__ key,
                                                      const unsigned char *__restrict__ tru, const int *__restrict__ run_off,
                                                      const unsigned long long *__restrict__ hardfn,
                                                      const unsigned *__restrict__ flags, int64_t *__restrict__ o_run_off,
                                                      int64_t *__restrict__ o_hardfn, unsigned *__restrict__ o_flags,
                                                      unsigned long long *__restrict__ o_key, unsigned *o_nt, unsigned *o_nf)
{
    __shared__ int wsum[17];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < NC; c += gridDim.x) {
        const int b = cell_off[c], n = cell_off[c + 1] - b;
        const int r0 = run_off[c], nr = run_off[c + 1] - r0;
        const unsigned long long *K = key + b;
        const unsigned char *T = tru + b;
        if (tid == 0) {
            o_run_off[c] = r0;
            if (c == NC - 1) o_run_off[NC] = run_off[NC];
            o_hardfn[c] = static_cast<int64_t>(hardfn[c]);
            o_flags[c] = flags[c];
        }
        int below = 0, nd = 0;  // true examples / runs before the tile
        for (int t0 = 0; t0 < n; t0 += 256) {
            const int i = t0 + tid;
            const bool in = i < n;
            const int tv = in ? T[i] : 0;
            const int first = in && (i == 0 || K[i] != K[i - 1]);
            int tt, tf;
            const int bt = ev_block_scan(tv, wsum, tt) + below;
            const int j = ev_block_scan(first, wsum, tf) + nd;
            if (first) {
                o_key[r0 + j] = K[i];
                o_nt[r0 + j] = static_cast<unsigned>(bt);
                o_nf[r0 + j] = static_cast<unsigned>(i - bt);
            }
            below += tt;
            nd += tf;
        }
        __syncthreads();  // the counts below every run are written
        for (int j0 = 0; j0 < nr; j0 += 256) {
            const int j = j0 + tid;
            unsigned dt = 0, df = 0;
            if (j < nr) {
                const unsigned et = j + 1 < nr ? o_nt[r0 + j + 1] : static_cast<unsigned>(below);
                const unsigned ef = j + 1 < nr ? o_nf[r0 + j + 1] : static_cast<unsigned>(n - below);
                dt = et - o_nt[r0 + j];
                df = ef - o_nf[r0 + j];
            }
            __syncthreads();  // entry j0 + 256 is read before the next tile overwrites it
            if (j < nr) {
                o_nt[r0 + j] = dt;
                o_nf[r0 + j] = df;
            }
        }
        __syncthreads();
    }
}

// a key ev_key gives for a score that is no NaN: -inf .. +inf, without the key of -0.0
__device__ __forceinline__ bool ev_key_ok(unsigned long long k)
{
    return k >= 0x000fffffffffffffull && k <= 0xfff0000000000000ull && k != 0x7fffffffffffffffull;
}

// The run checks of mc_ev_state_merge (run_off is checked by the host: from 0 ascending to R).
// flag[0]: 1 a run without examples, 2 a key of no score, 4 keys not strictly ascending within a
// cell; total: the examples of all runs.
__global__ __launch_bounds__(256) void k_ev_state_check(int NC, int64_t R, const int64_t *__restrict__ run_off,
                                                        const unsigned long long *__restrict__ key,
                                                        const unsigned *__restrict__ nt, const unsigned *__restrict__ nf,
                                                        int *__restrict__ flag, unsigned long long *__restrict__ total)
{
    int bad = 0;
    unsigned long long sum = 0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < R; i += static_cast<int64_t>(gridDim.x) * 256) {
        const unsigned long long n = static_cast<unsigned long long>(nt[i]) + nf[i];
        if (n == 0) bad |= 1;
        sum += n;
        const unsigned long long k = key[i];
        if (!ev_key_ok(k)) bad |= 2;
        int lo = 0, hi = NC;  // the cell of run i: the last c with run_off[c] <= i
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (run_off[mid] <= i) lo = mid;
            else hi = mid;
        }
        if (i > run_off[lo] && !(key[i - 1] < k)) bad |= 4;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        bad |= __shfl_xor(bad, d, 64);
        sum += __shfl_xor(sum, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicOr(&flag[0], bad);
        if (sum) atomicAdd(total, sum);
    }
}

// one workgroup of 1024: run_ex[R + 1], the examples before every run (their total is below 2^31)
__global__ __launch_bounds__(1024) void k_ev_state_scan(int R, const unsigned *__restrict__ nt, const unsigned *__restrict__ nf,
                                                        int *__restrict__ run_ex)
{
    __shared__ int wsum[17];
    const int ch = (R + 1023) / 1024;
    const int lo = min(R, static_cast<int>(threadIdx.x) * ch), hi = min(R, lo + ch);
    int n = 0;
    for (int i = lo; i < hi; i++) n += static_cast<int>(nt[i] + nf[i]);
    int tot;
    int at = ev_block_scan(n, wsum, tot);
    for (int i = lo; i < hi; i++) {
        run_ex[i] = at;
        at += static_cast<int>(nt[i] + nf[i]);
    }
    if (threadIdx.x == 0) run_ex[R] = tot;
}

// thread per example of the new region [0, run_ex[R]): its run by bisection, true for the run's first
// n_true examples
__global__ __launch_bounds__(256) void k_ev_state_expand(int R, const int *__restrict__ run_ex,
                                                         const unsigned long long *__restrict__ key,
                                                         const unsigned *__restrict__ nt, unsigned long long *__restrict__ ex_key,
                                                         unsigned char *__restrict__ ex_true)
{
    const int64_t n = run_ex[R];
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; e < n; e += static_cast<int64_t>(gridDim.x) * 256) {
        int lo = 0, hi = R;  // the last run with run_ex[r] <= e (runs are not empty)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (run_ex[mid] <= e) lo = mid;
            else hi = mid;
        }
        ex_key[e] = key[lo];
        ex_true[e] = (e - run_ex[lo] < static_cast<int64_t>(nt[lo])) ? 1 : 0;
    }
}

// thread per cell: hard false negatives and flags added; thread per non-empty cell of the buffer
// (cells[u], ascending): its examples as one unit
__global__ __launch_bounds__(256) void k_ev_state_units(int NC, int U, const int *__restrict__ cells,
                                                        const int64_t *__restrict__ run_off, const int *__restrict__ run_ex,
                                                        const int64_t *__restrict__ hardfn, const unsigned *__restrict__ flags,
                                                        int64_t ex_base, int *__restrict__ unit_cell, int *__restrict__ unit_cnt,
                                                        int64_t *__restrict__ unit_off, unsigned long long *__restrict__ cell_hardfn,
                                                        unsigned *__restrict__ cell_flags)
{
    for (int t = blockIdx.x * 256 + threadIdx.x; t < max(NC, U); t += gridDim.x * 256) {
        if (t < NC) {
            cell_hardfn[t] += static_cast<unsigned long long>(hardfn[t]);
            cell_flags[t] |= flags[t];
        }
        if (t < U) {
            const int c = cells[t];
            const int e0 = run_ex[run_off[c]], e1 = run_ex[run_off[c + 1]];
            unit_cell[t] = c;
            unit_cnt[t] = e1 - e0;
            unit_off[t] = ex_base + e0;
        }
    }
}

}  // namespace mc
