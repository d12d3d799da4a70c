// mc_s6_pairs.inl — S6: the edge rule and the pair kernels (supporter and observer counts, union at once);
// included by mc_kernels.inl after mc_s6_columns.inl.  Launched by s6_pairs and s6_pairs_dense
// (mc_cluster_host.inl).  Here are the edge capture (EdgeCap), the overflow work area (OvfWork, kOvfSlots),
// kPairWaves and the profiling knob MC_ABLATE_PAIRS.
namespace mc {

// Edge rule of update_graph (iterative_clustering.py:20-29) in float32, as torch evaluates
// it: disconnect if O < thr; connect if fl32(S / fl32(O + 1e-7f)) >= fl32(ct); i != j.
struct EdgeRule {
    float thr;  // observer_num_threshold (np.float32 or the int 1) as float32
    float ct;   // connect_threshold as float32
    int omin;   // smallest integer O with fl32(O) >= thr
    __device__ EdgeRule(float thr_, float ct_) : thr(thr_), ct(ct_)
    {
        omin = !(thr_ > 0.0f) ? 0 : (thr_ > 1.0e9f ? 1000000000 : static_cast<int>(ceilf(thr_)));
    }
};

__device__ __forceinline__ bool edge_ok(int o, int s, EdgeRule er)
{
    const float of = static_cast<float>(o);
    if (of < er.thr) return false;
    const float rate = __fdiv_rn(static_cast<float>(s), __fadd_rn(of, 1e-7f));
    return rate >= er.ct;
}

// Exact pre-filter on the supporter count alone: the rule is monotone non-increasing in O
// (int->float, +1e-7, S/x and every rounding are monotone), so if it fails at the smallest
// admissible O it fails for every O and the pair needs no observer count.
__device__ __forceinline__ bool edge_possible(int s, EdgeRule er) { return edge_ok(er.omin, s, er); }

// K4: supporter counts by sparse expansion (Gustavson row-by-row C·Cᵀ), one wave per node a:
//   S[a,b] = |C_a ∩ C_b| = #{m in C_a : b in col(m)}, accumulated in an LDS hash for b > a.
// Only pairs with S >= 1 can pass the rate test when ct > 0, so every candidate edge is
// enumerated.  Then O[a,b] = popcount(VF_a & VF_b) and the edge rule decide; edges are
// merged with union-find at once.  Loads are batched (independent gathers in flight
// before use); only the hash slots actually used are scanned and reset.
constexpr int kHashBits = 9, kHashSize = 1 << kHashBits, kHashMaxFill = (kHashSize * 3) / 4;
constexpr int kPairWaves = 4, kPairBatch = 8, kTestBatch = 4, kTestWords = 4;
// Profiling ablations (timing-only builds, results wrong): 1 = no union-find,
// 2 = no hash insert (expansion loads only), 3 = no partner test phase, 4 = no edge-count
// atomic, 5 = neither edge-count atomic nor union-find.
#ifndef MC_ABLATE_PAIRS
#define MC_ABLATE_PAIRS 0
#endif

// Optional capture of every edge (replay of the reference's set orders):
// key = t << 48 | a << 24 | b with a < b; buf == nullptr: off.
struct EdgeCap {
    unsigned long long *buf;
    unsigned long long *cnt;
    long long cap;
};
__device__ __forceinline__ void edge_capture(EdgeCap ec, int t, int a, int b)
{
    if (!ec.buf) return;
    const unsigned long long pos = atomicAdd(ec.cnt, 1ull);
    if (pos < static_cast<unsigned long long>(ec.cap))
        ec.buf[pos] = (static_cast<unsigned long long>(t) << 48) | (static_cast<unsigned long long>(a) << 24) |
                      static_cast<unsigned long long>(b);
}

// the same from a converged wave, one counter add per wave (every lane calls it; `e` = this lane
// has the edge (a, b))
__device__ __forceinline__ void edge_capture_wave(EdgeCap ec, int t, int a, int b, bool e)
{
    if (!ec.buf) return;
    const unsigned long long bal = __ballot(e);
    if (!bal) return;
    const int lane = static_cast<int>(threadIdx.x & 63);
    const int leader = __ffsll(static_cast<long long>(bal)) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(ec.cnt, static_cast<unsigned long long>(__popcll(bal)));
    base = __shfl(base, leader, 64);
    const unsigned long long pos = base + __popcll(bal & ((1ull << lane) - 1ull));
    if (e && pos < static_cast<unsigned long long>(ec.cap))
        ec.buf[pos] = (static_cast<unsigned long long>(t) << 48) | (static_cast<unsigned long long>(a) << 24) |
                      static_cast<unsigned long long>(b);
}

struct OvfWork {
    int *scratch, *touched;  // kOvfSlots dense counters / touched lists of N0 ints (zero at rest)
    int N0;
    int *locks;              // kOvfSlots slot locks (zero at rest)
};
constexpr int kOvfLocal = 256;  // overflow nodes per workgroup: <= 4 * ceil(N / (4 * 2048)) <= 128 for N <= 2^18

// K4b: nodes whose partner set overflowed the LDS hash, by a whole workgroup with dense global
// counters (scr[N0] zero on entry and on exit) and a touched list.
__device__ void pairs_overflow_node(int a, const int *__restrict__ n_off, const int *__restrict__ n_len,
                                    const int *__restrict__ pool, const int *__restrict__ coloff,
                                    const int *__restrict__ collen, const int *__restrict__ colnodes,
                                    const unsigned long long *__restrict__ nvf, int FW, EdgeRule er,
                                    int *__restrict__ parent, int *__restrict__ scr, int *__restrict__ tl,
                                    int *ntouch, unsigned long long &nedges, EdgeCap ec, int t)
{
    if (threadIdx.x == 0) *ntouch = 0;
    __syncthreads();
    const int o = n_off[a], L = n_len[a];
    for (int e = 0; e < L; e++) {
        const int m = pool[o + e];
        const int cb = coloff[m], ce = cb + collen[m];
        for (int k = cb + threadIdx.x; k < ce; k += 256) {
            const int bnode = colnodes[k];
            if (bnode <= a) continue;
            if (atomicAdd(&scr[bnode], 1) == 0) tl[atomicAdd(ntouch, 1)] = bnode;
        }
    }
    __syncthreads();
    const int nt = *ntouch;
    const unsigned long long *va = nvf + static_cast<size_t>(a) * FW;
    for (int k = threadIdx.x; k < nt; k += 256) {
        const int bnode = tl[k];
        const int sv = ld_agent(&scr[bnode]);
        st_agent(&scr[bnode], 0);
        if (!edge_possible(sv, er)) continue;
        const unsigned long long *vb = nvf + static_cast<size_t>(bnode) * FW;
        int ob = 0;
        for (int w = 0; w < FW; w++) ob += __popcll(va[w] & vb[w]);
        if (edge_ok(ob, sv, er)) {
            nedges++;
            edge_capture(ec, t, a, bnode);
            uf_unite(parent, a, bnode);
        }
    }
    // The clears are relaxed stores: a barrier alone lets them still be in flight when the next node's
    // adds, or (after the slot's release) another workgroup's, reach the same counters -- an add that finds
    // the old count does not list its partner, and the late clear wipes the adds.  Every thread has its
    // clears performed at device scope before the barrier.
    __threadfence();
    __syncthreads();
}

// Overflow nodes are redone inside k6_pairs' launch (no launch of its own) by the workgroup that
// listed them, once its own nodes are done, with one of kOvfSlots dense counter slots taken under
// a lock (rare: only workgroups with an overflowed node touch the locks).  The slots are shared by
// workgroups on different XCDs within one launch, so their counters are read and cleared with
// device-coherent accesses.
constexpr int kOvfSlots = 64;
__device__ void pairs_overflow_local(OvfWork ow, const int *ovf_nodes, int novf, const int *__restrict__ n_off,
                                     const int *__restrict__ n_len, const int *__restrict__ pool,
                                     const int *__restrict__ coloff, const int *__restrict__ collen,
                                     const int *__restrict__ colnodes, const unsigned long long *__restrict__ nvf,
                                     int FW, EdgeRule er, int *__restrict__ parent,
                                     unsigned long long *__restrict__ edges_t, EdgeCap ec, int t)
{
    __shared__ int s_slot, ntouch;
    __shared__ int ws[4];
    if (threadIdx.x == 0) {
        int slot = static_cast<int>(blockIdx.x % kOvfSlots);
        while (atomicCAS(&ow.locks[slot], 0, 1) != 0) {  // holders release without waiting on anyone
            slot = (slot + 1) % kOvfSlots;
            __builtin_amdgcn_s_sleep(2);
        }
        s_slot = slot;
    }
    __syncthreads();
    int *scr = ow.scratch + static_cast<size_t>(s_slot) * ow.N0;
    int *tl = ow.touched + static_cast<size_t>(s_slot) * ow.N0;
    unsigned long long nedges = 0;
    for (int q = 0; q < novf; q++)
        pairs_overflow_node(ovf_nodes[q], n_off, n_len, pool, coloff, collen, colnodes, nvf, FW, er, parent, scr, tl,
                            &ntouch, nedges, ec, t);
    const int ne = block_sum<256>(static_cast<int>(nedges), ws);  // (every thread's clears are fenced; its barriers put them before the release)
    if (threadIdx.x == 0) {
        if (ne) spread_add(edges_t, static_cast<unsigned long long>(ne));
        atomicExch(&ow.locks[s_slot], 0);
    }
}

// K4 (described above, before its constants); its overflowed nodes go to K4b at the end of the launch
__global__ __launch_bounds__(256) void k6_pairs(const int *__restrict__ dN, const int *__restrict__ n_off,
                                                const int *__restrict__ n_len, const int *__restrict__ pool,
                                                const int *__restrict__ coloff, const int *__restrict__ collen,
                                                const int *__restrict__ colnodes,
                                                const unsigned long long *__restrict__ nvf, int FW,
                                                const float *__restrict__ thr, int t, float ctf,
                                                int *__restrict__ parent, unsigned long long *__restrict__ edges,
                                                OvfWork ow, int shard_rank, int shard_world, EdgeCap ec)
{
    __shared__ int s_ovf[kOvfLocal];
    __shared__ int s_novf;
    __shared__ int hkey[kPairWaves][kHashSize];
    __shared__ int hcnt[kPairWaves][kHashSize];
    __shared__ short hused[kPairWaves][kHashMaxFill + 64];
    __shared__ int epre[kPairWaves][65];
    __shared__ int ebeg[kPairWaves][64];
    __shared__ int hfill[kPairWaves];
    __shared__ int hovf[kPairWaves];

    const int N = *dN;
    const int wv = threadIdx.x >> 6, lane = lane_id();
    const EdgeRule er{thr[t], ctf};
    int *keys = hkey[wv];
    int *cnts = hcnt[wv];
    short *used = hused[wv];
    unsigned long long nedges = 0;

    // rows a = shard_rank (mod shard_world): the row-block share of this process
    if ((blockIdx.x * kPairWaves) * shard_world + shard_rank >= N) return;  // uniform: nothing for this block
    if (threadIdx.x == 0) s_novf = 0;
    for (int s = lane; s < kHashSize; s += 64) {
        keys[s] = -1;
        cnts[s] = 0;
    }
    sync_global();
    for (int a = (blockIdx.x * kPairWaves + wv) * shard_world + shard_rank; a < N;
         a += gridDim.x * kPairWaves * shard_world) {
        if (lane == 0) {
            hfill[wv] = 0;
            hovf[wv] = 0;
        }
        wave_sync();
        const int o = n_off[a], L = n_len[a];
        for (int e0 = 0; e0 < L; e0 += 64) {
            const int e = e0 + lane;
            int len = 0, beg = 0;
            if (e < L) {
                const int m = pool[o + e];
                beg = coloff[m];
                len = collen[m];
            }
            const int incl = wave_incl_scan(len);
            epre[wv][lane + 1] = incl;
            ebeg[wv][lane] = beg;
            if (lane == 0) epre[wv][0] = 0;
            wave_sync();
            const int total = __shfl(incl, 63, 64);
            for (int k0 = 0; k0 < total; k0 += 64 * kPairBatch) {
                int bn[kPairBatch];
#pragma unroll
                for (int r = 0; r < kPairBatch; r++) {
                    const int k = k0 + r * 64 + lane;
                    bn[r] = -1;
                    if (k < total) {
                        int lo = 0;  // largest entry with epre[lo] <= k
#pragma unroll
                        for (int st = 32; st >= 1; st >>= 1)
                            if (epre[wv][lo + st] <= k) lo += st;
                        bn[r] = colnodes[ebeg[wv][lo] + (k - epre[wv][lo])];
                    }
                }
#pragma unroll
                for (int r = 0; r < kPairBatch; r++) {
                    const int bnode = bn[r];
                    if (bnode <= a || hovf[wv]) continue;
                    if (MC_ABLATE_PAIRS == 2) {
                        asm volatile("" ::"v"(bnode));
                        continue;
                    }
                    unsigned h = (static_cast<unsigned>(bnode) * 2654435761u) >> (32 - kHashBits);
                    for (int probe = 0; probe < kHashSize; probe++) {
                        int cur = keys[h];
                        if (cur == -1) {
                            cur = atomicCAS(&keys[h], -1, bnode);
                            if (cur == -1) {
                                const int f = atomicAdd(&hfill[wv], 1);
                                if (f >= kHashMaxFill) hovf[wv] = 1;
                                else used[f] = static_cast<short>(h);
                                cur = bnode;
                            }
                        }
                        if (cur == bnode) {
                            atomicAdd(&cnts[h], 1);
                            break;
                        }
                        h = (h + 1) & (kHashSize - 1);
                    }
                }
            }
            wave_sync();
        }
        wave_sync();
        const int fill = min(hfill[wv], kHashMaxFill);
        const bool ovf = hovf[wv] != 0;
        if (ovf && lane == 0) s_ovf[atomicAdd(&s_novf, 1)] = a;  // redone by the whole workgroup below
        const unsigned long long *va = nvf + static_cast<size_t>(a) * FW;
        if (ovf) {
            // clear every slot (inserted keys past the used list are not tracked)
            for (int s = lane; s < kHashSize; s += 64) {
                keys[s] = -1;
                cnts[s] = 0;
            }
        } else if (MC_ABLATE_PAIRS != 3) {
            for (int x0 = 0; x0 < fill; x0 += 64 * kTestBatch) {
                int bn[kTestBatch], sc[kTestBatch], ob[kTestBatch];
#pragma unroll
                for (int r = 0; r < kTestBatch; r++) {
                    const int x = x0 + r * 64 + lane;
                    bn[r] = -1;
                    sc[r] = 0;
                    ob[r] = 0;
                    if (x < fill) {
                        const int sl = used[x];
                        bn[r] = keys[sl];
                        sc[r] = cnts[sl];
                        keys[sl] = -1;
                        cnts[sl] = 0;
                        if (!edge_possible(sc[r], er)) bn[r] = -1;
                    }
                }
                for (int w0 = 0; w0 < FW; w0 += kTestWords) {  // all words of a chunk in flight at once
                    unsigned long long aw[kTestWords], bw[kTestBatch][kTestWords];
#pragma unroll
                    for (int j = 0; j < kTestWords; j++) aw[j] = w0 + j < FW ? va[w0 + j] : 0ull;
#pragma unroll
                    for (int r = 0; r < kTestBatch; r++)
#pragma unroll
                        for (int j = 0; j < kTestWords; j++)
                            bw[r][j] = (bn[r] >= 0 && w0 + j < FW) ? nvf[static_cast<size_t>(bn[r]) * FW + w0 + j] : 0ull;
#pragma unroll
                    for (int r = 0; r < kTestBatch; r++)
#pragma unroll
                        for (int j = 0; j < kTestWords; j++) ob[r] += __popcll(aw[j] & bw[r][j]);
                }
#pragma unroll
                for (int r = 0; r < kTestBatch; r++) {
                    const bool e = bn[r] >= 0 && edge_ok(ob[r], sc[r], er);
                    edge_capture_wave(ec, t, a, bn[r], e);
                    if (e) {
                        nedges++;
                        if (MC_ABLATE_PAIRS != 1 && MC_ABLATE_PAIRS != 5) uf_unite(parent, a, bn[r]);
                    }
                }
            }
        } else {
            for (int x = lane; x < fill; x += 64) {
                const int sl = used[x];
                keys[sl] = -1;
                cnts[sl] = 0;
            }
        }
        wave_sync();
    }
    // wave-reduce the edge count
    int ne = static_cast<int>(nedges);
    ne = wave_sum(ne);
    if (MC_ABLATE_PAIRS < 4 && lane == 0 && ne)
        spread_add(edges + static_cast<size_t>(t) * kSpread * kSpreadStrideL, static_cast<unsigned long long>(ne));
    sync_global();
    if (s_novf > 0)  // uniform
        pairs_overflow_local(ow, s_ovf, s_novf, n_off, n_len, pool, coloff, collen, colnodes, nvf, FW, er, parent,
                             edges + static_cast<size_t>(t) * kSpread * kSpreadStrideL, ec, t);
}

// Dense observer-only pairs for ct <= 0 (every pair with O >= thr is an edge, S unused).
__global__ __launch_bounds__(256) void k6_pairs_dense(const int *__restrict__ dN,
                                                      const unsigned long long *__restrict__ nvf, int FW,
                                                      const float *__restrict__ thr, int t, int *__restrict__ parent,
                                                      unsigned long long *__restrict__ edges, EdgeCap ec)
{
    __shared__ int ws[4];
    const int N = *dN;
    const float thr_f = thr[t];
    unsigned long long nedges = 0;
    const long long npairs = static_cast<long long>(N) * N;
    for (long long q = blockIdx.x * 256ll + threadIdx.x; q < npairs; q += gridDim.x * 256ll) {
        const int a = static_cast<int>(q / N), b = static_cast<int>(q % N);
        if (b <= a) continue;
        int ob = 0;
        for (int w = 0; w < FW; w++) ob += __popcll(nvf[static_cast<size_t>(a) * FW + w] & nvf[static_cast<size_t>(b) * FW + w]);
        if (!(static_cast<float>(ob) < thr_f)) {  // ct <= 0: every rate >= ct
            nedges++;
            edge_capture(ec, t, a, b);
            uf_unite(parent, a, b);
        }
    }
    int ne = block_sum<256>(static_cast<int>(nedges), ws);
    if (threadIdx.x == 0 && ne) spread_add(edges + static_cast<size_t>(t) * kSpread * kSpreadStrideL, static_cast<unsigned long long>(ne));
}

}  // namespace mc
