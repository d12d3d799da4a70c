// mc_scan.inl — device exclusive scans and their host launchers (included by mc_kernels.inl; used by every
// stage): scan_device_n (one workgroup, n read on the device), scan_device_multi (many workgroups, n read on
// the device, up to two arrays) and scan_large (many workgroups, host-known n).
namespace mc {

// Exclusive scan of n ints (n read from *dn when dn != nullptr) by ONE 1024-thread workgroup.
// out[0..n] gets n+1 entries (out[n] = total); *dtotal = total when given.  Up to two
// independent arrays per launch (in2/out2 may be null).  Tiles of 8192 ints are staged
// through LDS so global loads and stores are coalesced; LDS index padded (i + i/32).
constexpr int kScan1Tile = 8192;
__device__ __forceinline__ int scan_pad(int i) { return i + (i >> 5); }

__global__ __launch_bounds__(1024) void k_scan1(const int *__restrict__ in, int *__restrict__ out, const int *dn,
                                                int n_host, int *dtotal, const int *__restrict__ in2,
                                                int *__restrict__ out2, int *dtotal2)
{
    __shared__ int buf[kScan1Tile + kScan1Tile / 32];
    __shared__ int ws[16];
    const int n = dn ? *dn : n_host;
    constexpr int IT = kScan1Tile / 1024;
    for (int arr = 0; arr < 2; arr++) {
        const int *src = arr == 0 ? in : in2;
        int *dst = arr == 0 ? out : out2;
        int *tot_out = arr == 0 ? dtotal : dtotal2;
        if (!src) break;
        int carry = 0;
        for (int base = 0; base < n; base += kScan1Tile) {
            const int cnt = min(kScan1Tile, n - base);
            for (int i = threadIdx.x; i < kScan1Tile; i += 1024) buf[scan_pad(i)] = i < cnt ? src[base + i] : 0;
            __syncthreads();
            int v[IT];
            int s = 0;
#pragma unroll
            for (int k = 0; k < IT; k++) {
                v[k] = buf[scan_pad(threadIdx.x * IT + k)];
                s += v[k];
            }
            int tot;
            int ex = block_excl_scan<1024>(s, ws, tot) + carry;
#pragma unroll
            for (int k = 0; k < IT; k++) {
                buf[scan_pad(threadIdx.x * IT + k)] = ex;
                ex += v[k];
            }
            __syncthreads();
            for (int i = threadIdx.x; i < cnt; i += 1024) dst[base + i] = buf[scan_pad(i)];
            carry += tot;
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            dst[n] = carry;
            if (tot_out) *tot_out = carry;
        }
    }
}

// Multi-block exclusive scan for large host-known n (the P-length degree scan).
constexpr int kScanBlock = 256, kScanItems = 16, kScanTile = kScanBlock * kScanItems;

__global__ __launch_bounds__(256) void k_scan_reduce(const int *__restrict__ in, int n, int *__restrict__ partial)
{
    __shared__ int ws[4];
    const int i0 = blockIdx.x * kScanTile;
    int s = 0;
    for (int k = threadIdx.x; k < kScanTile; k += 256) {
        int i = i0 + k;
        s += i < n ? in[i] : 0;
    }
    s = block_sum<256>(s, ws);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_scan_down(const int *__restrict__ in, int n, const int *__restrict__ pscan,
                                                   int *__restrict__ out)
{
    __shared__ int ws[4];
    const int i0 = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    int v[kScanItems];
    int s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        v[k] = (i0 + k < n) ? in[i0 + k] : 0;
        s += v[k];
    }
    int tot;
    int ex = block_excl_scan<256>(s, ws, tot) + pscan[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        if (i0 + k < n) out[i0 + k] = ex;
        ex += v[k];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[n] = pscan[gridDim.x];
}

void scan_device_n(hipStream_t s, const int *in, int *out, const int *dn, int n_host, int *dtotal,
                   const int *in2 = nullptr, int *out2 = nullptr, int *dtotal2 = nullptr)
{
    hipLaunchKernelGGL(k_scan1, dim3(1), dim3(1024), 0, s, in, out, dn, n_host, dtotal, in2, out2, dtotal2);
}

// The same by many workgroups with n read from the device (*dn, bounded by the host's n_cap): block
// sums, one single-workgroup scan of them, each block's tile; up to two arrays (blockIdx.y), each
// with out[n] = total and *dtotal = total.  For the per-batch S1 scans (~10^5 ints), which the
// single-workgroup k_scan1 walks one 8192-int tile after another.
struct ScanArrays {
    const int *in[2];
    int *out[2];
    int *dtotal[2];
};
__global__ __launch_bounds__(256) void k_scanm_reduce(ScanArrays a, const int *dn, int n_host, int *__restrict__ partial)
{
    __shared__ int ws[4];
    const int n = dn ? *dn : n_host;
    const int *in = a.in[blockIdx.y];
    const int i0 = blockIdx.x * kScanTile;
    int s = 0;
    if (i0 < n)  // (uniform in the block)
        for (int k = threadIdx.x; k < kScanTile; k += 256) {
            const int i = i0 + k;
            s += i < n ? in[i] : 0;
        }
    s = block_sum<256>(s, ws);
    if (threadIdx.x == 0) partial[blockIdx.y * (gridDim.x + 1) + blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_scanm_down(ScanArrays a, const int *dn, int n_host, const int *__restrict__ pscan)
{
    __shared__ int ws[4];
    const int n = dn ? *dn : n_host;
    const int y = blockIdx.y;
    const int *ps = pscan + y * (gridDim.x + 1);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.out[y][n] = ps[gridDim.x];
        if (a.dtotal[y]) *a.dtotal[y] = ps[gridDim.x];
    }
    if (static_cast<int>(blockIdx.x) * kScanTile >= n) return;  // (uniform in the block)
    const int *in = a.in[y];
    int *out = a.out[y];
    const int i0 = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    int v[kScanItems];
    int s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        v[k] = (i0 + k < n) ? in[i0 + k] : 0;
        s += v[k];
    }
    int tot;
    int ex = block_excl_scan<256>(s, ws, tot) + ps[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kScanItems; k++) {
        if (i0 + k < n) out[i0 + k] = ex;
        ex += v[k];
    }
}
// tmp: >= 4 * (n_cap / kScanTile + 2) ints
void scan_device_multi(hipStream_t s, const int *dn, int n_cap, int *tmp, const int *in, int *out, int *dtotal,
                       const int *in2 = nullptr, int *out2 = nullptr, int *dtotal2 = nullptr)
{
    const int nb = std::max(1, ceil_div(n_cap, kScanTile));
    if (nb <= 2) {
        scan_device_n(s, in, out, dn, n_cap, dtotal, in2, out2, dtotal2);
        return;
    }
    const int ny = in2 ? 2 : 1;
    const ScanArrays a{{in, in2}, {out, out2}, {dtotal, dtotal2}};
    int *part = tmp, *pscan = tmp + 2 * (nb + 1);
    hipLaunchKernelGGL(k_scanm_reduce, dim3(nb, ny), dim3(256), 0, s, a, dn, n_cap, part);
    scan_device_n(s, part, pscan, nullptr, nb, nullptr, ny > 1 ? part + nb + 1 : nullptr,
                  ny > 1 ? pscan + nb + 1 : nullptr, nullptr);
    hipLaunchKernelGGL(k_scanm_down, dim3(nb, ny), dim3(256), 0, s, a, dn, n_cap, pscan);
}

void scan_large(hipStream_t s, const int *in, int *out, int n, int *tmp /* >= 2*(n/tile+2) */)
{
    const int nb = ceil_div(n, kScanTile);
    if (nb <= 1) {
        scan_device_n(s, in, out, nullptr, n, nullptr);
        return;
    }
    hipLaunchKernelGGL(k_scan_reduce, dim3(nb), dim3(256), 0, s, in, n, tmp);
    scan_device_n(s, tmp, tmp + nb + 1, nullptr, nb, nullptr);
    hipLaunchKernelGGL(k_scan_down, dim3(nb), dim3(256), 0, s, in, n, tmp + nb + 1, out);
}

}  // namespace mc
