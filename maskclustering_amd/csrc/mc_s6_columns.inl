// mc_s6_columns.inl — S6 iterative clustering (graph/iterative_clustering.py:5-43, graph/node.py:24-37),
// first part: the union-find and the column lists (the nodes that contain each mask); included by
// mc_kernels.inl.  Launched by s6_level0_columns and s6_pairs_dense (mc_cluster_host.inl); the per-level
// column update (col_update_block, ColUpdate) runs inside k6_merge's launch (mc_s6_merge.inl).
namespace mc {

// union-find over a parent array in global memory, device-scope accesses
// (uf_find_s / uf_unite_s, mc_bp_denoise_common.inl, restate it for an LDS array)
__device__ __forceinline__ int uf_find(int *parent, int x)
{
    while (true) {
        const int p = ld_agent(parent + x);
        if (p == x) return x;
        const int gp = ld_agent(parent + p);
        if (gp == p) return p;
        st_agent(parent + x, gp);  // path halving; gp is an ancestor of x
        x = gp;
    }
}

// Hook the larger root under the smaller one: every root is its component's minimum.
__device__ __forceinline__ void uf_unite(int *parent, int a, int b)
{
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        if (atomicCAS(parent + b, b, a) == b) return;
    }
}

// K1: parent init + column counts (nodes that contain mask m), one thread per pool slot.
__global__ __launch_bounds__(256) void k6_colcount(const int *__restrict__ dN, const int *__restrict__ dcap,
                                                   const int *__restrict__ pool, const int *__restrict__ owner,
                                                   int *__restrict__ parent, int *__restrict__ colcnt)
{
    const int N = *dN, cap = *dcap;
    const int lim = max(N, cap);
    for (int e = blockIdx.x * 256 + threadIdx.x; e < lim; e += gridDim.x * 256) {
        if (e < N) parent[e] = e;
        if (e < cap && owner[e] >= 0) atomicAdd(&colcnt[pool[e]], 1);
    }
}

__global__ __launch_bounds__(256) void k6_parent_init(const int *__restrict__ dN, int *__restrict__ parent)
{
    const int N = *dN;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) parent[i] = i;
}

// K3: column lists (transpose of the node-mask incidence); colcnt returns to zero.
__global__ __launch_bounds__(256) void k6_colscatter(const int *__restrict__ dcap, const int *__restrict__ pool,
                                                     const int *__restrict__ owner, const int *__restrict__ coloff,
                                                     int *__restrict__ colcnt, int *__restrict__ colnodes)
{
    const int cap = *dcap;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < cap; e += gridDim.x * 256) {
        const int a = owner[e];
        if (a < 0) continue;
        const int m = pool[e];
        colnodes[coloff[m] + atomicSub(&colcnt[m], 1) - 1] = a;
    }
}

// Column lists of the next level in place (iteration t >= 1): every column m keeps its
// level-0 slot range [coloff[m], coloff[m+1]) and a current length collen[m]; its node
// ids are mapped through the previous iteration's labels, sorted and deduplicated
// (a column is the set of nodes contained by mask m).  label == nullptr: initialise
// the lengths after the level-0 transpose.  Also resets the union-find parents.
constexpr int kColStage = 2048;
constexpr int kColLaneMax = 64;  // unstaged columns up to this length are sorted by their own lane
__device__ __forceinline__ int col_sort_unique(int *c, int n)
{
    for (int i = 1; i < n; i++) {
        const int x = c[i];
        int j = i - 1;
        while (j >= 0 && c[j] > x) {
            c[j + 1] = c[j];
            j--;
        }
        c[j + 1] = x;
    }
    int u = 0;
    for (int j = 0; j < n; j++)
        if (u == 0 || c[j] != c[u - 1]) c[u++] = c[j];
    return u;
}

// the columns [64 blk, 64 blk + 64) by one wave (lane = column), staged in LDS when they fit
__device__ __forceinline__ void col_update_block(int blk, int Mn, const int *__restrict__ coloff,
                                                 int *__restrict__ collen, int *__restrict__ colnodes,
                                                 const int *__restrict__ label, int *stage)
{
    const int lane = lane_id();
    const int m0 = blk * 64, m1 = min(Mn, m0 + 64);
    const int m = m0 + lane;
    if (!label) {
        if (m < m1) collen[m] = coloff[m + 1] - coloff[m];
        return;
    }
    const int eb = coloff[m0], ee = coloff[m1];
    if (ee - eb <= kColStage) {
        for (int x = lane; x < ee - eb; x += 64) stage[x] = colnodes[eb + x];
        wave_sync();
        if (m < m1) {
            int *c = stage + coloff[m] - eb;
            const int n = collen[m];
            for (int j = 0; j < n; j++) c[j] = label[c[j]];
            collen[m] = col_sort_unique(c, n);
        }
        wave_sync();
        for (int x = lane; x < ee - eb; x += 64) colnodes[eb + x] = stage[x];
        wave_sync();
    } else {
        // the group does not fit the stage: its columns one at a time, by the whole wave, as a
        // sorted-unique set through an LDS bitmap over the column's label range (one lane per
        // column only when that range exceeds the bitmap)
        unsigned *bm = reinterpret_cast<unsigned *>(stage);
        // short columns in their own lanes (global memory), long ones by the whole wave below
        const int nl = m < m1 ? collen[m] : 0;
        if (m < m1 && nl <= kColLaneMax) {
            int *c = colnodes + coloff[m];
            for (int j = 0; j < nl; j++) c[j] = label[c[j]];
            collen[m] = col_sort_unique(c, nl);
        }
        unsigned long long longs = __ballot(m < m1 && nl > kColLaneMax);
        while (longs) {
            const int mm = m0 + __ffsll(static_cast<long long>(longs)) - 1;
            longs &= longs - 1;
            int *c = colnodes + coloff[mm];
            const int n = collen[mm];
            int lo = INT_MAX, hi = -1;
            for (int j = lane; j < n; j += 64) {
                const int l = label[c[j]];
                lo = min(lo, l);
                hi = max(hi, l);
            }
            lo = wave_min_i(lo);
            hi = wave_max_i(hi);
            if (n == 0) continue;
            const int RW = ((hi - lo) >> 5) + 1;
            if (RW > kColStage) {
                if (lane == 0) {
                    for (int j = 0; j < n; j++) c[j] = label[c[j]];
                    collen[mm] = col_sort_unique(c, n);
                }
                wave_sync();
                continue;
            }
            for (int w = lane; w < RW; w += 64) bm[w] = 0u;
            wave_sync();
            for (int j = lane; j < n; j += 64) {
                const int l = label[c[j]] - lo;
                atomicOr(&bm[l >> 5], 1u << (l & 31));
            }
            wave_sync();
            int pos = 0;
            for (int w0 = 0; w0 < RW; w0 += 64) {
                const unsigned v = w0 + lane < RW ? bm[w0 + lane] : 0u;
                const int cnt = __popc(v);
                const int incl = wave_incl_scan(cnt);
                int o = pos + incl - cnt;
                unsigned x = v;
                while (x) {
                    const int bt = __ffs(x) - 1;
                    x &= x - 1;
                    c[o++] = lo + ((w0 + lane) << 5) + bt;
                }
                pos += __shfl(incl, 63, 64);
            }
            if (lane == 0) collen[mm] = pos;
            wave_sync();
        }
    }
}

// one wave per 64 columns (level-0 lengths; k6_merge carries the per-iteration update)
__global__ __launch_bounds__(64) void k6_colupdate(int Mn, const int *__restrict__ dN, const int *__restrict__ coloff,
                                                   int *__restrict__ collen, int *__restrict__ colnodes,
                                                   const int *__restrict__ label, int *__restrict__ parent)
{
    __shared__ int stage[kColStage];
    const int N = *dN;
    const int nblk_cols = (Mn + 63) / 64;
    for (int i = blockIdx.x * 64 + threadIdx.x; i < N; i += gridDim.x * 64) parent[i] = i;
    for (int blk = blockIdx.x; blk < nblk_cols; blk += gridDim.x)
        col_update_block(blk, Mn, coloff, collen, colnodes, label, stage);
}

// The next iteration's column update, folded into k6_merge's launch (it needs only this
// iteration's labels, which k6_merge does not touch): before the K merge items come
// ceil(ceil(Mn/64)/4) column items of four 64-column groups, one per wave, staged in the
// merge bitmap's LDS; the union-find parents of the next level are reset too.
struct ColUpdate {
    int Mn;
    const int *dN;  // next level's node count (parents to reset)
    const int *coloff;
    int *collen, *colnodes;
    const int *label;  // this iteration's labels; null: no column update
    int *parent;
    int N0;             // level-0 nodes: final_label[i] = level_label[final_label[i]]
    const int *level_label;
    int *final_label;
};

}  // namespace mc
