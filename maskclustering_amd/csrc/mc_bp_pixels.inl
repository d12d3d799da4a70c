// mc_bp_pixels.inl — S1 back-projection, bp_launch_pixels: valid pixels per (frame, id), the candidate
// slots and their pixel lists.
namespace mc {

// ---------------------------------------------------------------------------------------------
// (a2) pixels -> masks
// ---------------------------------------------------------------------------------------------
// One block per (band of kBpBand rows, frame); wave w of the block owns sub-band w (kBpSub rows).
// band_cnt[f][sub-band][id]: valid-depth pixels of id in the sub-band (0 < d < trunc: Open3D keeps
// d < trunc, :22; ids != 0, :94); present[f]: ids in the image (torch.unique, :77); fflags[f]: 1 =
// a pixel with d == trunc (the reference's IndexError at :100), 2 = inf in the pose (:73-74, frame
// skipped).
constexpr int kBpWaves = 4;                   // waves (= sub-bands) per band block
constexpr int kBpSub = kBpBand / kBpWaves;    // rows per sub-band
constexpr int kBpPix = 4;                     // 64-pixel steps whose loads a wave issues together
__global__ __launch_bounds__(256) void k_bp_count(const float *__restrict__ depth, const unsigned char *__restrict__ seg,
                                                  const double *__restrict__ pose, BpDev pr, int *__restrict__ band_cnt,
                                                  unsigned *__restrict__ present, int *__restrict__ fflags,
                                                  unsigned char *__restrict__ vid)
{
    __shared__ int cnt[kBpWaves][256];
    __shared__ unsigned pres[8];
    __shared__ int sflag;
    const int f = blockIdx.y, band = blockIdx.x, t = threadIdx.x, lane = lane_id(), wv = t >> 6;
    const int W = pr.W;
#pragma unroll
    for (int w = 0; w < kBpWaves; w++) cnt[w][t] = 0;
    if (t < 8) pres[t] = 0u;
    if (t == 0) sflag = 0;
    __syncthreads();
    if (t < 16 && isinf(pose[16 * static_cast<size_t>(f) + t])) atomicOr(&sflag, 2);
    __syncthreads();
    const bool skip = (sflag & 2) != 0;
    const size_t fb = static_cast<size_t>(f) * pr.H * W;
    const int sb = band * kBpWaves + wv;  // this wave's sub-band
    const int i0 = min(pr.H, sb * kBpSub) * W, i1 = min(pr.H, (sb + 1) * kBpSub) * W;
    int trunc = 0, lastp = -1;
    if (pr.vec4) {  // four consecutive pixels per lane: one 4-byte seg load and one 16-byte depth load
      for (int ib0 = i0; ib0 < i1; ib0 += 256 * 2) {
        uchar4 sv[2];
        float4 dq[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const int i = ib0 + 256 * u + 4 * lane;
          sv[u] = i < i1 ? *reinterpret_cast<const uchar4 *>(seg + fb + i) : make_uchar4(0, 0, 0, 0);
          dq[u] = i < i1 ? *reinterpret_cast<const float4 *>(depth + fb + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const int i = ib0 + 256 * u + 4 * lane;
          const int sids[4] = {sv[u].x, sv[u].y, sv[u].z, sv[u].w};
          const float ds[4] = {dq[u].x, dq[u].y, dq[u].z, dq[u].w};
          unsigned vw = 0u;  // the four pixels' valid ids (k_bp_compact reads these instead of seg + depth)
          int id[4];
          unsigned pend = 0u;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            id[j] = -1;
            if (i < i1) {
                const int sid = sids[j];
                const float d = ds[j];
                if (sid != lastp) {
                    atomicOr(&pres[sid >> 5], 1u << (sid & 31));
                    lastp = sid;
                }
                if (static_cast<double>(d) == pr.trunc) trunc = 1;
                if (sid != 0 && !skip && d > 0.0f && static_cast<double>(d) < pr.trunc) id[j] = sid;
            }
            vw |= static_cast<unsigned>(id[j] > 0 ? id[j] : 0) << (8 * j);
            if (id[j] >= 0) pend |= 1u << j;
          }
          // one LDS add per distinct id of the wave's 256 pixels: each lane's count of the id among
          // its four pixels (0..4) summed over the wave from three ballots of the count's bits
          while (true) {
            const unsigned long long act = __ballot(pend != 0u);
            if (!act) break;
            const int L = __ffsll(static_cast<long long>(act)) - 1;
            int mine = -1;
#pragma unroll
            for (int j = 3; j >= 0; j--)
              if (pend & (1u << j)) mine = id[j];
            const int k = __builtin_amdgcn_readlane(mine, L);
            unsigned mb = 0u;
#pragma unroll
            for (int j = 0; j < 4; j++)
              if ((pend & (1u << j)) && id[j] == k) mb |= 1u << j;
            const int c = __popc(mb);
            const int tot = __popcll(__ballot(c & 1)) + 2 * __popcll(__ballot(c & 2)) + 4 * __popcll(__ballot(c & 4));
            if (lane == L) cnt[wv][k] += tot;
            pend &= ~mb;
          }
          if (i < i1) *reinterpret_cast<unsigned *>(vid + fb + i) = vw;
        }
      }
    } else
    for (int ib0 = i0; ib0 < i1; ib0 += 64 * kBpPix) {
      // kBpPix steps' loads issued before the first is used
      int sidv[kBpPix];
      float dv[kBpPix];
#pragma unroll
      for (int u = 0; u < kBpPix; u++) {
        const int i = ib0 + 64 * u + lane;
        sidv[u] = i < i1 ? seg[fb + i] : 0;
        dv[u] = i < i1 ? depth[fb + i] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kBpPix; u++) {
        const int i = ib0 + 64 * u + lane;
        int id = -1;
        if (i < i1) {
            const int sid = sidv[u];
            const float d = dv[u];
            if (sid != lastp) {
                atomicOr(&pres[sid >> 5], 1u << (sid & 31));
                lastp = sid;
            }
            if (static_cast<double>(d) == pr.trunc) trunc = 1;
            if (sid != 0 && !skip && d > 0.0f && static_cast<double>(d) < pr.trunc) id = sid;
            vid[fb + i] = static_cast<unsigned char>(id > 0 ? id : 0);
        }
        unsigned long long act = __ballot(id >= 0);
        while (act) {  // one LDS add per distinct id per wave
            const int leader = __ffsll(static_cast<long long>(act)) - 1;
            const int k = __shfl(id, leader, 64);
            const unsigned long long m = __ballot(id == k);
            if (lane == leader) cnt[wv][k] += __popcll(m);  // the wave's own row
            act &= ~m;
        }
      }
    }
    if (trunc) atomicOr(&sflag, 1);
    __syncthreads();
    const size_t nsb = static_cast<size_t>(pr.nbands) * kBpWaves;
#pragma unroll
    for (int w = 0; w < kBpWaves; w++) band_cnt[(static_cast<size_t>(f) * nsb + band * kBpWaves + w) * 256 + t] = cnt[w][t];
    if (t < 8 && pres[t]) atomicOr(&present[f * 8 + t], pres[t]);
    if (t == 0 && sflag) atomicOr(&fflags[f], sflag);
}

// One block per frame, 1024 threads = id x quarter: sub-band counts -> sub-band offsets within the id's
// pixel list (each quarter of the sub-bands summed with eight loads in flight, the quarters' totals
// scanned through LDS); candidate = id != 0 with >= few_points valid pixels (:101) in a frame that
// neither returns early (inf pose) nor raises (d == trunc with ids present; *err_frame = first such
// frame).
__global__ __launch_bounds__(1024) void k_bp_frames(int *__restrict__ band_cnt, const unsigned *__restrict__ present,
                                                    const int *__restrict__ fflags, BpDev pr, int *__restrict__ cand,
                                                    int *__restrict__ npix, int *__restrict__ err_frame)
{
    __shared__ int qsum[4][256];
    const int f = blockIdx.x, id = threadIdx.x & 255, qt = threadIdx.x >> 8;
    const int fl = fflags[f];
    bool any_id = false;
    for (int w = 0; w < 8; w++) any_id |= (present[f * 8 + w] & (w == 0 ? ~1u : ~0u)) != 0u;
    const bool inf_pose = (fl & 2) != 0;
    const bool err = !inf_pose && any_id && (fl & 1);
    if (err && threadIdx.x == 0) atomicMin(err_frame, f);
    const int nsb = pr.nbands * kBpWaves;
    const int per = (nsb + 3) / 4, b0 = min(nsb, qt * per), b1 = min(nsb, b0 + per);
    int *bc = band_cnt + static_cast<size_t>(f) * nsb * 256 + id;
    // this quarter's total, eight sub-bands' loads issued together
    int tot = 0;
    for (int b = b0; b < b1; b += 8) {
        int c[8];
#pragma unroll
        for (int u = 0; u < 8; u++) c[u] = b + u < b1 ? bc[static_cast<size_t>(b + u) * 256] : 0;
#pragma unroll
        for (int u = 0; u < 8; u++) tot += c[u];
    }
    qsum[qt][id] = tot;
    __syncthreads();
    int run = 0;
    for (int k = 0; k < qt; k++) run += qsum[k][id];
    // exclusive offsets of this quarter's sub-bands
    for (int b = b0; b < b1; b += 8) {
        int c[8];
#pragma unroll
        for (int u = 0; u < 8; u++) c[u] = b + u < b1 ? bc[static_cast<size_t>(b + u) * 256] : 0;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (b + u < b1) bc[static_cast<size_t>(b + u) * 256] = run;
            run += c[u];
        }
    }
    if (qt == 3) {  // run = the id's total in the frame
        const bool ok = id != 0 && !inf_pose && !err && run >= pr.few;
        cand[f * 256 + id] = ok ? 1 : 0;
        npix[f * 256 + id] = ok ? run : 0;
    }
}

__global__ __launch_bounds__(256) void k_bp_slots(const int *__restrict__ cand, const int *__restrict__ sidx,
                                                  const int *__restrict__ npix, const int *__restrict__ poff, int n,
                                                  int *__restrict__ slot_of, int *__restrict__ slot_frame,
                                                  int *__restrict__ slot_id, int *__restrict__ slot_np,
                                                  int *__restrict__ slot_pix, const int *__restrict__ npx, int px_cap,
                                                  int *__restrict__ dNS, int *__restrict__ ovf)
{
    // more mask pixels than the pixel-list capacity: no slot (the compaction writes nothing, every later
    // kernel sees zero slots); the host grows the arrays and redoes the batch
    const bool over = *npx >= px_cap;
    if (over && blockIdx.x == 0 && threadIdx.x == 0) {
        *dNS = 0;
        *ovf = 1;
    }
    for (int x = blockIdx.x * 256 + threadIdx.x; x < n; x += gridDim.x * 256) {
        if (cand[x] && !over) {
            const int s = sidx[x];
            slot_frame[s] = x >> 8;
            slot_id[s] = x & 255;
            slot_np[s] = npix[x];
            slot_pix[s] = poff[x];
            slot_of[x] = s;
        } else {
            slot_of[x] = -1;
        }
    }
}

// Stable compaction: every slot's pixels in row-major order (the order of view_points[valid_mask],
// :96-100).  Each wave walks its own sub-band with its own per-id cursors (the sub-band offsets of
// k_bp_frames), ranks within a 64-pixel step by ballot groups: no barrier after the set-up.  The
// pixels come from k_bp_count's valid-id map (1 byte per pixel: the id where the depth is valid, else
// 0), not from the frames' seg + depth (5 bytes).
__global__ __launch_bounds__(256) void k_bp_compact(const unsigned char *__restrict__ vid,
                                                    const int *__restrict__ band_off, const int *__restrict__ slot_of,
                                                    const int *__restrict__ slot_pix, BpDev pr,
                                                    unsigned *__restrict__ pix_list)
{
    __shared__ int cur[kBpWaves][256];
    const int f = blockIdx.y, band = blockIdx.x, t = threadIdx.x, lane = lane_id(), wv = t >> 6;
    const int W = pr.W;
    const size_t nsb = static_cast<size_t>(pr.nbands) * kBpWaves;
    {
        const int s = slot_of[f * 256 + t];
        const int sp = s >= 0 ? slot_pix[s] : -1;
#pragma unroll
        for (int w = 0; w < kBpWaves; w++)
            cur[w][t] = s >= 0 ? sp + band_off[(static_cast<size_t>(f) * nsb + band * kBpWaves + w) * 256 + t] : -1;
    }
    __syncthreads();
    const size_t fb = static_cast<size_t>(f) * pr.H * W;
    const int sb = band * kBpWaves + wv;
    const int i0 = min(pr.H, sb * kBpSub) * W, i1 = min(pr.H, (sb + 1) * kBpSub) * W;
    int *mycur = cur[wv];
    if (pr.vec4) {
      // four consecutive pixels per lane (lane-major: pixel = 4 * lane + j of the 256-pixel step);
      // per id: each lane counts its matching pixels, a wave exclusive scan of the counts gives
      // the lanes' bases, the leader bumps the cursor by the total
      for (int ib0 = i0; ib0 < i1; ib0 += 256 * 4) {
        uchar4 sv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int i = ib0 + 256 * u + 4 * lane;
          sv[u] = i < i1 ? *reinterpret_cast<const uchar4 *>(vid + fb + i) : make_uchar4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int i = ib0 + 256 * u + 4 * lane;
          const int sids[4] = {sv[u].x, sv[u].y, sv[u].z, sv[u].w};
          int id[4];
          unsigned pend = 0u;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            id[j] = -1;
            if (i < i1) {
                const int sid = sids[j];  // valid-id map of k_bp_count: 0 = no id or no valid depth
                if (sid != 0 && mycur[sid] >= 0) id[j] = sid;
            }
            if (id[j] >= 0) pend |= 1u << j;
          }
          int pos[4] = {0, 0, 0, 0};
          while (true) {
            const unsigned long long act = __ballot(pend != 0u);
            if (!act) break;
            const int L = __ffsll(static_cast<long long>(act)) - 1;
            int mine = -1;
#pragma unroll
            for (int j = 3; j >= 0; j--)
              if (pend & (1u << j)) mine = id[j];
            const int k = __builtin_amdgcn_readlane(mine, L);
            unsigned mb = 0u;
#pragma unroll
            for (int j = 0; j < 4; j++)
              if ((pend & (1u << j)) && id[j] == k) mb |= 1u << j;
            const int c = __popc(mb);
            // the lanes' exclusive prefix of c (0..4) and its total from three ballots of c's bits
            const unsigned long long below = (1ull << lane) - 1ull;
            const unsigned long long c0 = __ballot(c & 1), c1 = __ballot(c & 2), c2 = __ballot(c & 4);
            const int excl = __popcll(c0 & below) + 2 * __popcll(c1 & below) + 4 * __popcll(c2 & below);
            const int tot = __popcll(c0) + 2 * __popcll(c1) + 4 * __popcll(c2);
            int b = 0;
            if (lane == L) {
              b = mycur[k];
              mycur[k] = b + tot;
            }
            b = __builtin_amdgcn_readlane(b, L) + excl;
#pragma unroll
            for (int j = 0; j < 4; j++)
              if (mb & (1u << j)) pos[j] = b + __popc(mb & ((1u << j) - 1u));
            pend &= ~mb;
          }
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (id[j] >= 0) pix_list[pos[j]] = static_cast<unsigned>(i + j);
        }
      }
      return;
    }
    for (int ib0 = i0; ib0 < i1; ib0 += 64 * kBpPix) {
      int sidv[kBpPix];
#pragma unroll
      for (int u = 0; u < kBpPix; u++) {
        const int i = ib0 + 64 * u + lane;
        sidv[u] = i < i1 ? vid[fb + i] : 0;
      }
#pragma unroll
      for (int u = 0; u < kBpPix; u++) {
        const int i = ib0 + 64 * u + lane;
        int id = -1;
        if (i < i1) {
            const int sid = sidv[u];
            if (sid != 0 && mycur[sid] >= 0) id = sid;
        }
        unsigned long long act = __ballot(id >= 0);
        int pos = 0;
        while (act) {
            const int L = __ffsll(static_cast<long long>(act)) - 1;
            const int k = __shfl(id, L, 64);
            const unsigned long long m = __ballot(id == k);
            int b = 0;
            if (lane == L) {
                b = mycur[k];
                mycur[k] = b + __popcll(m);
            }
            b = __shfl(b, L, 64);
            if (id == k) pos = b + __popcll(m & ((1ull << lane) - 1ull));
            act &= ~m;
        }
        if (id >= 0) pix_list[pos] = static_cast<unsigned>(i);
      }
    }
}

}  // namespace mc
