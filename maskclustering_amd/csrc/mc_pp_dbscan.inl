// mc_pp_dbscan.inl — dbscan_process (utils/post_process.py:104-123): pp_dbscan of mc_pp_host.inl.
// Included by mc_pp_kernels.inl.
//
// DBSCAN of every node (:109): labels -> object index within the node (class order: noise first when
// present, then clusters by smallest core point), object sizes.  Two routes run the same steps, each
// written once below (pp_grid, pp_point_count, pp_point_unions, pp_ranks, pp_labels):
//   k_pp_dbscan      a node per workgroup: the neighbour walk over bucket-ordered copies (PPWalkSorted),
//                    the union-find in LDS while the node fits (kPPLdsUF);
//   k_pp_big_grid, k_pp_big_walk<0 / 1>, k_pp_big_label
//                    a node above the host's threshold (e.g. a floor of ScanNet++ size) split over many
//                    workgroups: its grid by one workgroup, the neighbour counts and the core-point
//                    unions on (node, 512-point chunk) items over the whole chip, ranks / labels /
//                    objects again per node; the walk over the bucket list (PPWalkList), the union-find
//                    in global memory.
// The routes differ in the walk and in where the union-find lives, and in nothing else.

namespace mc {

__global__ __launch_bounds__(256) void k_pp_gather(const double *__restrict__ scene, const int *__restrict__ pts, int64_t E,
                                                   double *__restrict__ xyz)
{
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < 3 * E; i += gridDim.x * 256ll)
        xyz[i] = scene[3 * static_cast<int64_t>(pts[i / 3]) + i % 3];
}

// the per-entry scratch arrays of every node, as pp_dbscan reserves them
struct PPNodes {
    const int64_t *pt_off;
    const double *xyz;
    unsigned long long *pcell;
    int *pbkt, *bcnt, *bstart, *blist, *ncnt, *par, *root, *rnk, *lab, *ccnt;
    int *nob, *nsh;  // per node: objects, class -> object shift
    int *gcm;        // per node: cmax[3], from k_pp_big_grid to the split route's later kernels
    unsigned long long *skey;  // k_pp_dbscan's bucket-ordered copies of the cell keys, points and indices
    double *sxyz;
    int *sidx;
};

// node k's part of them
struct PPNode {
    int k, n;
    int64_t e0;
    unsigned nb;  // hash buckets
    const double *P;
    unsigned long long *pc;
    int *pb, *bc, *bs, *bl, *nc, *pa, *ro, *rk, *lb, *cc;
};

__device__ __forceinline__ PPNode pp_node(const PPNodes &b, int k)
{
    PPNode d;
    d.k = k;
    d.e0 = b.pt_off[k];
    d.n = static_cast<int>(b.pt_off[k + 1] - d.e0);
    d.nb = 2u * static_cast<unsigned>(d.n);
    d.P = b.xyz + 3 * d.e0;
    d.pc = b.pcell + d.e0;
    d.pb = b.pbkt + d.e0;
    d.bc = b.bcnt + 2 * d.e0 + k;
    d.bs = b.bstart + 2 * d.e0 + k;
    d.bl = b.blist + d.e0;
    d.nc = b.ncnt + d.e0;
    d.pa = b.par + d.e0;
    d.ro = b.root + d.e0;
    d.rk = b.rnk + d.e0;
    d.lb = b.lab + d.e0;
    d.cc = b.ccnt + d.e0 + k;
    return d;
}

__device__ __forceinline__ BpCells pp_cells(const PPNode &d, const int *cmax)
{
    BpCells g;
    g.pc = d.pc;
    g.bs = d.bs;
    g.bl = d.bl;
    g.nb = d.nb;
#pragma unroll
    for (int c = 0; c < 3; c++) g.cmax[c] = cmax[c];
    return g;
}

// the 27 cells around (cx, cy, cz) over the bucket-ordered copies (key, xyz, index): the loads of
// one bucket are independent of each other, not a cell -> point -> coordinate chain
template <typename Fn>
__device__ __forceinline__ void pp_walk27(const BpCells &g, const unsigned long long *__restrict__ sk,
                                          const double *__restrict__ sx, const int *__restrict__ si, int cx, int cy,
                                          int cz, Fn &&fn)
{
    for (int z = cz - 1; z <= cz + 1; z++)
        for (int y = cy - 1; y <= cy + 1; y++)
            for (int x = cx - 1; x <= cx + 1; x++) {
                if (x < 0 || y < 0 || z < 0 || x > g.cmax[0] || y > g.cmax[1] || z > g.cmax[2]) continue;
                const unsigned long long key = pack3(x, y, z);
                const unsigned bk = mod_mul(bp_hash3(x, y, z), g.nb);
                const int k1 = g.bs[bk + 1];
                for (int q = g.bs[bk]; q < k1; q++)
                    if (sk[q] == key) fn(si[q], sx + 3 * static_cast<int64_t>(q));
            }
}

// The two neighbour walks: walk(i, fn) calls fn(j, pj) for every point j (at pj) in the 27 cells around
// point i's.  The two layouts are deliberate (pp_walk27's comment; the split route has no copies).
struct PPWalkSorted {
    BpCells g;
    const unsigned long long *sk;
    const double *sx;
    const int *si;
    template <typename Fn>
    __device__ __forceinline__ void operator()(int i, Fn &&fn) const
    {
        int x, y, z;
        unpack3(g.pc[i], x, y, z);
        pp_walk27(g, sk, sx, si, x, y, z, fn);
    }
};
struct PPWalkList {
    BpCells g;
    const double *P;
    template <typename Fn>
    __device__ __forceinline__ void operator()(int i, Fn &&fn) const
    {
        int x, y, z;
        unpack3(g.pc[i], x, y, z);
        for (int R = 0; R <= 1; R++) bp_shell(g, x, y, z, R, [&](int j) { fn(j, P + 3 * j); });
    }
};

// Exclusive scan of val(i), i < m, by the workgroup in NT-wide tiles with a carry: put(i, val(i), sum
// before i) for every i < m; returns the total.  ws holds NT/64 ints.
template <int NT, typename Val, typename Put>
__device__ __forceinline__ int pp_scan_tiles(int m, int *ws, Val &&val, Put &&put)
{
    int carry = 0;
    for (int i0 = 0; i0 < m; i0 += NT) {
        const int i = i0 + static_cast<int>(threadIdx.x);
        const int v = i < m ? val(i) : 0;
        int tot;
        const int ex = block_excl_scan<NT>(v, ws, tot);
        if (i < m) put(i, v, carry + ex);
        carry += tot;
    }
    return carry;
}

// Steps 1-4, the node's grid: bounding box -> grid origin and cmax (cells of 1.01 eps: every
// eps-neighbour is in the 27 cells), cell keys and bucket counts, bucket starts, counting-sort scatter.
// each(i) runs once per point beside its cell key; placed(i, q) when point i takes place q of the
// bucket order.  The bucket counters are zero at rest and return to zero; the class counters are cleared.
template <int NT, typename Each, typename Placed>
__device__ __forceinline__ void pp_grid(const PPNode &d, const PPDev &pr, double *red, int *ws, int cmax[3],
                                        Each &&each, Placed &&placed)
{
    const int t = threadIdx.x, n = d.n;
    const double *P = d.P;
    double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, mx[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    for (int i = t; i < n; i += NT)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            mn[c] = fmin(mn[c], P[3 * i + c]);
            mx[c] = fmax(mx[c], P[3 * i + c]);
        }
    pp_block_minmax3<NT>(mn, mx, red);
#pragma unroll
    for (int c = 0; c < 3; c++) cmax[c] = static_cast<int>(floor((mx[c] - mn[c]) / pr.ce));
    for (int i = t; i < n; i += NT) {
        int cxyz[3];
#pragma unroll
        for (int c = 0; c < 3; c++) cxyz[c] = static_cast<int>(floor((P[3 * i + c] - mn[c]) / pr.ce));
        d.pc[i] = pack3(cxyz[0], cxyz[1], cxyz[2]);
        const unsigned b = mod_mul(bp_hash3(cxyz[0], cxyz[1], cxyz[2]), d.nb);
        d.pb[i] = static_cast<int>(b);
        atomicAdd(&d.bc[b], 1);
        each(i);
    }
    for (int i = t; i <= n; i += NT) d.cc[i] = 0;
    sync_global();
    const int total = pp_scan_tiles<NT>(
        static_cast<int>(d.nb), ws, [&](int b) { return ld_agent(&d.bc[b]); }, [&](int b, int, int at) { d.bs[b] = at; });
    if (t == 0) d.bs[d.nb] = total;
    sync_global();
    for (int i = t; i < n; i += NT) {
        const int b = d.pb[i];
        const int q = d.bs[b] + atomicSub(&d.bc[b], 1) - 1;
        d.bl[q] = i;
        placed(i, q);
    }
    sync_global();
}

// Step 5 for point i: its eps-neighbour count, self included (nanoflann radius search: d2 < eps^2)
template <typename Walk>
__device__ __forceinline__ int pp_point_count(const PPNode &d, const PPDev &pr, int i, Walk &&walk)
{
    int cnt = 0;
    const double *pi = d.P + 3 * i;
    walk(i, [&](int, const double *pj) { cnt += bp_d2(pi, pj) < pr.eps2 ? 1 : 0; });
    return cnt;
}

// Step 6 for core point i: unite(i, j) with every core point j < i within eps (root = smallest index)
template <typename Walk, typename Unite>
__device__ __forceinline__ void pp_point_unions(const PPNode &d, const PPDev &pr, int i, Walk &&walk, Unite &&unite)
{
    const double *pi = d.P + 3 * i;
    walk(i, [&](int j, const double *pj) {
        if (j < i && d.nc[j] >= pr.minpts && bp_d2(pi, pj) < pr.eps2) unite(i, j);
    });
}

// Step 7: the root of every core point; clusters numbered by their smallest core point (Open3D seeds
// in index order).  Returns the number of clusters.
template <int NT, typename Find>
__device__ __forceinline__ int pp_ranks(const PPNode &d, const PPDev &pr, int *ws, Find &&find)
{
    const int ncl = pp_scan_tiles<NT>(
        d.n, ws,
        [&](int i) {
            if (d.nc[i] < pr.minpts) return 0;
            const int r = find(i);
            d.ro[i] = r;
            return r == i ? 1 : 0;
        },
        [&](int i, int isr, int at) {
            if (isr) d.rk[i] = at;
        });
    sync_global();
    return ncl;
}

// Steps 8 and 9.  Labels: a border point joins the first cluster that reaches it = the adjacent cluster
// of smallest number, noise when there is none; class = label + 1 (post_process.py:109).  Objects =
// non-empty classes (:115-118): the noise class only when it is non-empty; object = class - shift.
template <int NT, typename Walk>
__device__ __forceinline__ void pp_labels(const PPNode &d, const PPDev &pr, int ncl, int *nob, int *nsh, Walk &&walk)
{
    const int t = threadIdx.x;
    for (int i = t; i < d.n; i += NT) {
        int l;
        if (d.nc[i] >= pr.minpts) {
            l = d.rk[d.ro[i]];
        } else {
            const double *pi = d.P + 3 * i;
            int mr = INT_MAX;
            walk(i, [&](int j, const double *pj) {
                if (d.nc[j] >= pr.minpts && bp_d2(pi, pj) < pr.eps2) mr = min(mr, d.ro[j]);
            });
            l = mr == INT_MAX ? -1 : d.rk[mr];
        }
        d.lb[i] = l + 1;
        atomicAdd(&d.cc[l + 1], 1);
    }
    sync_global();
    if (t == 0) {
        const int noise = ld_agent(&d.cc[0]) > 0 ? 1 : 0;
        nob[d.k] = ncl + noise;
        nsh[d.k] = 1 - noise;
    }
    sync_global();
}

// a node per workgroup, taken largest-first from the ticket
template <int NT>
__global__ __launch_bounds__(NT) void k_pp_dbscan(int N, const int *__restrict__ order, int *__restrict__ ticket, PPDev pr,
                                                  PPNodes b)
{
    __shared__ double red[6 * (NT / 64)];
    __shared__ int ws[NT / 64];
    __shared__ int s_k;
    __shared__ int s_par[kPPLdsUF];  // union-find in LDS when the node fits: global-memory find chains
                                     // (a dependent load per step) made the unions the whole cost
    const int t = threadIdx.x;
    while (true) {
        if (t == 0) s_k = atomicAdd(ticket, 1);
        sync_global();
        const int kk = s_k;
        sync_global();
        if (kk >= N) break;
        const PPNode d = pp_node(b, order[kk]);
        const int n = d.n;
        unsigned long long *sk = b.skey + d.e0;
        double *sx = b.sxyz + 3 * d.e0;
        int *si = b.sidx + d.e0;
        int cmax[3];
        pp_grid<NT>(
            d, pr, red, ws, cmax, [](int) {},
            [&](int i, int q) {
                sk[q] = d.pc[i];
                si[q] = i;
#pragma unroll
                for (int c = 0; c < 3; c++) sx[3 * q + c] = d.P[3 * i + c];
            });
        const PPWalkSorted walk{pp_cells(d, cmax), sk, sx, si};
        for (int i = t; i < n; i += NT) {
            d.nc[i] = pp_point_count(d, pr, i, walk);
            if (n <= kPPLdsUF) s_par[i] = i;
            else d.pa[i] = i;
        }
        sync_global();
        for (int i = t; i < n; i += NT) {
            if (d.nc[i] < pr.minpts) continue;
            pp_point_unions(d, pr, i, walk, [&](int a, int c) {
                if (n <= kPPLdsUF) uf_unite_s(s_par, a, c);
                else uf_unite(d.pa, a, c);
            });
        }
        sync_global();
        const int ncl = pp_ranks<NT>(d, pr, ws, [&](int i) { return n <= kPPLdsUF ? uf_find_s(s_par, i) : uf_find(d.pa, i); });
        pp_labels<NT>(d, pr, ncl, b.nob, b.nsh, walk);
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void k_pp_big_grid(int nbig, const int *__restrict__ big, PPDev pr, PPNodes b)
{
    __shared__ double red[6 * (NT / 64)];
    __shared__ int ws[NT / 64];
    for (int q = blockIdx.x; q < nbig; q += gridDim.x) {
        const PPNode d = pp_node(b, big[q]);
        int cmax[3];
        pp_grid<NT>(
            d, pr, red, ws, cmax, [&](int i) { d.pa[i] = i; }, [](int, int) {});
        if (threadIdx.x == 0)
#pragma unroll
            for (int c = 0; c < 3; c++) b.gcm[3 * d.k + c] = cmax[c];
    }
}

// PASS 0: eps-neighbour counts; PASS 1: unions of core points
template <int NT, int PASS>
__global__ __launch_bounds__(NT) void k_pp_big_walk(int nitems, const int2 *__restrict__ items, PPDev pr, PPNodes b)
{
    for (int q = blockIdx.x; q < nitems; q += gridDim.x) {
        const PPNode d = pp_node(b, items[q].x);
        const int i = items[q].y + static_cast<int>(threadIdx.x);
        if (i >= d.n) continue;
        const PPWalkList walk{pp_cells(d, b.gcm + 3 * d.k), d.P};
        if (PASS == 0) {
            d.nc[i] = pp_point_count(d, pr, i, walk);
        } else {
            if (d.nc[i] < pr.minpts) continue;
            pp_point_unions(d, pr, i, walk, [&](int a, int c) { uf_unite(d.pa, a, c); });
        }
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void k_pp_big_label(int nbig, const int *__restrict__ big, PPDev pr, PPNodes b)
{
    __shared__ int ws[NT / 64];
    for (int q = blockIdx.x; q < nbig; q += gridDim.x) {
        const PPNode d = pp_node(b, big[q]);
        const PPWalkList walk{pp_cells(d, b.gcm + 3 * d.k), d.P};
        const int ncl = pp_ranks<NT>(d, pr, ws, [&](int i) { return uf_find(d.pa, i); });
        pp_labels<NT>(d, pr, ncl, b.nob, b.nsh, walk);
    }
}

}  // namespace mc
