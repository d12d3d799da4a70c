// mc_s6_merge.inl — S6: components of the union-find forest, relabelling, the merge of every component's
// rows into the next level, and the start of S6 (k6_init); included by mc_kernels.inl after mc_s6_pairs.inl.
// Launched by s6_components, s6_merge and s6_init (mc_cluster_host.inl).
namespace mc {

// Multi-workgroup K5-K9 (large N: level 0, and every level of very large scenes).
// K5: root of every node; flag roots (= smallest member of each component).
// Also clears the row-length accumulator of the next level and the overflow count.
__global__ __launch_bounds__(256) void k6_compress(const int *__restrict__ dN, int *__restrict__ parent,
                                                   int *__restrict__ root, int *__restrict__ isroot,
                                                   int *__restrict__ ublen, int *__restrict__ ovf_n)
{
    const int N = *dN;
    if (blockIdx.x == 0 && threadIdx.x == 0) *ovf_n = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
        const int r = uf_find(parent, i);
        root[i] = r;
        isroot[i] = r == i ? 1 : 0;
        ublen[i] = 0;
    }
}

// K7: label = rank of the component's smallest member — the order of
// nx.connected_components (iterative_clustering.py:7); member counts and
// an upper bound of every new row length (sum of member lengths).
__global__ __launch_bounds__(256) void k6_relabel(const int *__restrict__ dN, const int *__restrict__ root,
                                                  const int *__restrict__ rank, const int *__restrict__ n_len,
                                                  int *__restrict__ label, int *__restrict__ level_out,
                                                  int *__restrict__ memcnt, int *__restrict__ ublen)
{
    const int N = *dN;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
        const int k = rank[root[i]];
        label[i] = k;
        level_out[i] = k;
        atomicAdd(&memcnt[k], 1);
        atomicAdd(&ublen[k], n_len[i]);
    }
}

// K9: members of every new node (memcnt returns to zero) + object of every level-0 node.
__global__ __launch_bounds__(256) void k6_memscatter(const int *__restrict__ dN, int N0, const int *__restrict__ label,
                                                     const int *__restrict__ memoff, int *__restrict__ memcnt,
                                                     int *__restrict__ members, int *__restrict__ final_label)
{
    const int N = *dN;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < max(N, N0); i += gridDim.x * 256) {
        if (i < N) {
            const int k = label[i];
            members[memoff[k] + atomicSub(&memcnt[k], 1) - 1] = i;
        }
        if (i < N0) final_label[i] = label[final_label[i]];
    }
}

// K5-K9 in one 1024-thread workgroup (one launch instead of five; every step is O(N)):
// roots and their ranks in index order (the component order of nx.connected_components,
// iterative_clustering.py:7), labels, member counts and row-length bounds, their scans (member
// offsets, next-level row offsets, next N and pool capacity) and the member lists.  Every
// thread owns a contiguous index range, so each scan is one block scan of per-thread totals.
// memcnt is zero on entry and on exit.  (The level-0 objects are relabelled in k6_merge.)
__device__ __forceinline__ int2 block_excl_scan2(int a, int b, int *ws, int &ta, int &tb)
{
    const int ea = block_excl_scan<1024>(a, ws, ta);
    const int eb = block_excl_scan<1024>(b, ws, tb);
    return make_int2(ea, eb);
}

__global__ __launch_bounds__(1024) void k6_components(
    const int *__restrict__ dN, int *__restrict__ dNn, int *__restrict__ parent, int *__restrict__ root,
    int *__restrict__ rank, const int *__restrict__ n_len, int *__restrict__ label, int *__restrict__ level_out,
    int *__restrict__ memcnt, int *__restrict__ memoff, int *__restrict__ ublen, int *__restrict__ newoff,
    int *__restrict__ dcap_next, int *__restrict__ members, int *__restrict__ ovf_n)
{
    __shared__ int ws[16];
    const int N = *dN;
    const int t = threadIdx.x;
    if (t == 0) *ovf_n = 0;
    const int per = (N + 1023) / 1024;
    const int i0 = min(N, t * per), i1 = min(N, i0 + per);
    // roots (own range), then ranks of the roots in index order
    int nr = 0;
    for (int i = i0; i < i1; i++) {
        const int r = uf_find(parent, i);
        root[i] = r;
        ublen[i] = 0;
        nr += r == i ? 1 : 0;
    }
    int K;
    int rk = block_excl_scan<1024>(nr, ws, K);
    for (int i = i0; i < i1; i++)
        if (root[i] == i) rank[i] = rk++;
    sync_global();  // root / rank / counters / offsets are read by other waves
    // labels, member counts, row-length upper bounds
    for (int i = t; i < N; i += 1024) {
        const int k = rank[root[i]];
        label[i] = k;
        level_out[i] = k;
        atomicAdd(&memcnt[k], 1);
        atomicAdd(&ublen[k], n_len[i]);
    }
    sync_global();  // root / rank / counters / offsets are read by other waves
    // member offsets and next-level row offsets (K + 1 entries each)
    const int pk = (K + 1023) / 1024;
    const int k0 = min(K, t * pk), k1 = min(K, k0 + pk);
    int s0 = 0, s1 = 0;
    for (int k = k0; k < k1; k++) {
        s0 += ld_agent(&memcnt[k]);
        s1 += ld_agent(&ublen[k]);
    }
    int T0, T1;
    int2 e = block_excl_scan2(s0, s1, ws, T0, T1);
    for (int k = k0; k < k1; k++) {
        memoff[k] = e.x;
        newoff[k] = e.y;
        e.x += ld_agent(&memcnt[k]);
        e.y += ld_agent(&ublen[k]);
    }
    if (t == 0) {
        memoff[K] = T0;
        newoff[K] = T1;
        *dcap_next = T1;
        *dNn = K;
    }
    sync_global();  // root / rank / counters / offsets are read by other waves
    // members of every new node (memcnt returns to zero)
    for (int i = t; i < N; i += 1024) {
        const int k = label[i];
        members[memoff[k] + atomicSub(&memcnt[k], 1) - 1] = i;
    }
}

// K10: new node k = OR of its members (node.py:33-34): C row as a sorted unique union
// (LDS bitmap over the members' [lo, hi] mask range), VF as OR of member VF words.
// Rows are written at upper-bound offsets; the unused tail of every range gets owner -1.
constexpr int kMergeBitWords = 8192;  // LDS bitmap: 262,144 mask ids
constexpr int kMaxFW = 256;           // F <= 16384

__global__ __launch_bounds__(256) void k6_merge(const int *__restrict__ dK, const int *__restrict__ memoff,
                                                const int *__restrict__ members, const int *__restrict__ n_off,
                                                const int *__restrict__ n_len, const int *__restrict__ pool,
                                                const unsigned long long *__restrict__ nvf, int FW,
                                                const int *__restrict__ newoff, int *__restrict__ nn_off,
                                                int *__restrict__ nn_len, int *__restrict__ npool,
                                                int *__restrict__ nowner, unsigned long long *__restrict__ nnvf,
                                                ColUpdate cu)
{
    static_assert(4 * kColStage <= kMergeBitWords, "column stages alias the merge bitmap");
    __shared__ unsigned bits[kMergeBitWords];
    __shared__ unsigned long long vacc[kMaxFW];
    __shared__ int ws[4];
    __shared__ int s_lo, s_hi;
    const int K = *dK;
    const int ncolblk = cu.label ? (cu.Mn + 63) / 64 : 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cu.N0; i += gridDim.x * 256)
        cu.final_label[i] = cu.level_label[cu.final_label[i]];  // object of every level-0 node
    if (cu.label) {
        const int Nn = *cu.dN;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < Nn; i += gridDim.x * 256) cu.parent[i] = i;
    }
    const int ncolitems = (ncolblk + 3) / 4;  // first, so that they spread over the first grid round
    for (int item = blockIdx.x; item < ncolitems + K; item += gridDim.x) {
        if (item < ncolitems) {  // uniform per block
            const int blk = 4 * item + static_cast<int>(threadIdx.x >> 6);
            if (blk < ncolblk)
                col_update_block(blk, cu.Mn, cu.coloff, cu.collen, cu.colnodes, cu.label,
                                 reinterpret_cast<int *>(bits) + (threadIdx.x >> 6) * kColStage);
            __syncthreads();
            continue;
        }
        const int k = item - ncolitems;
        const int mb = memoff[k], me = memoff[k + 1];
        const int dst = newoff[k], dend = newoff[k + 1];
        if (me - mb == 1) {
            for (int w = threadIdx.x; w < FW; w += 256)
                nnvf[static_cast<size_t>(k) * FW + w] = nvf[static_cast<size_t>(members[mb]) * FW + w];
        } else {
            for (int w = threadIdx.x; w < FW; w += 256) vacc[w] = 0ull;
            __syncthreads();
            const int nmw = (me - mb) * FW;
            for (int x = threadIdx.x; x < nmw; x += 256) {
                const int q = mb + x / FW, w = x % FW;
                const unsigned long long v = nvf[static_cast<size_t>(members[q]) * FW + w];
                if (v) atomicOr(&vacc[w], v);
            }
            __syncthreads();
            for (int w = threadIdx.x; w < FW; w += 256) nnvf[static_cast<size_t>(k) * FW + w] = vacc[w];
        }
        if (me - mb == 1) {
            const int i = members[mb];
            const int o = n_off[i], l = n_len[i];
            for (int x = threadIdx.x; x < l; x += 256) {
                npool[dst + x] = pool[o + x];
                nowner[dst + x] = k;
            }
            if (threadIdx.x == 0) {
                nn_off[k] = dst;
                nn_len[k] = l;
            }
            continue;  // uniform branch
        }
        if (threadIdx.x == 0) {
            s_lo = INT_MAX;
            s_hi = -1;
        }
        __syncthreads();
        for (int q = mb + threadIdx.x; q < me; q += 256) {
            const int i = members[q];
            const int l = n_len[i];
            if (l > 0) {
                atomicMin(&s_lo, pool[n_off[i]]);
                atomicMax(&s_hi, pool[n_off[i] + l - 1]);
            }
        }
        __syncthreads();
        const int lo = s_lo, hi = s_hi;
        if (hi < lo) {  // all members have empty rows
            for (int x = dst + threadIdx.x; x < dend; x += 256) nowner[x] = -1;
            if (threadIdx.x == 0) {
                nn_off[k] = dst;
                nn_len[k] = 0;
            }
            __syncthreads();
            continue;
        }
        const int RW = ((hi - lo) >> 5) + 1;  // <= kMergeBitWords (checked at setup: M <= 262144)
        for (int w = threadIdx.x; w < RW; w += 256) bits[w] = 0u;
        __syncthreads();
        for (int q = mb; q < me; q++) {
            const int i = members[q];
            const int o = n_off[i], l = n_len[i];
            for (int x = threadIdx.x; x < l; x += 256) {
                const int m = pool[o + x] - lo;
                atomicOr(&bits[m >> 5], 1u << (m & 31));
            }
        }
        __syncthreads();
        // ordered extraction: thread t owns a contiguous chunk of words
        const int per = (RW + 255) / 256;
        const int w0 = threadIdx.x * per, w1 = min(RW, w0 + per);
        int mine = 0;
        for (int w = w0; w < w1; w++) mine += __popc(bits[w]);
        int tot;
        int pos = block_excl_scan<256>(mine, ws, tot) + dst;
        for (int w = w0; w < w1; w++) {
            unsigned v = bits[w];
            while (v) {
                const int bt = __ffs(v) - 1;
                v &= v - 1;
                nowner[pos] = k;
                npool[pos++] = lo + (w << 5) + bt;
            }
        }
        for (int x = dst + tot + threadIdx.x; x < dend; x += 256) nowner[x] = -1;
        if (threadIdx.x == 0) {
            nn_off[k] = dst;
            nn_len[k] = tot;
        }
        __syncthreads();
    }
}

// Start of S6: final_label = identity, level-0 size, edge counters.
__global__ __launch_bounds__(256) void k6_init(int N0, int *__restrict__ final_label, const int *__restrict__ n0_src,
                                               int n0_host, int *__restrict__ Nlev, int *__restrict__ cap0,
                                               const int *__restrict__ cap_src, int cap_host,
                                               unsigned long long *__restrict__ edges, int nthr)
{
    const int i0 = blockIdx.x * 256 + threadIdx.x;
    if (i0 == 0) {
        *Nlev = n0_src ? *n0_src : n0_host;
        *cap0 = cap_src ? *cap_src : cap_host;
    }
    for (int i = i0; i < nthr * kSpread; i += gridDim.x * 256) edges[static_cast<size_t>(i) * kSpreadStrideL] = 0ull;
    for (int i = i0; i < N0; i += gridDim.x * 256) final_label[i] = i;
}

}  // namespace mc
