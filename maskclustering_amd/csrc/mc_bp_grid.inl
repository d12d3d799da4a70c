// mc_bp_grid.inl — S1 back-projection: the scene's hashed grid, built once per scene by bp_build_grid
// and read by the ball query of every bp_run after it (mc_bp_query.inl).
namespace mc {

// ---------------------------------------------------------------------------------------------
// scene grid (built once per scene): points bucketed by cells of 2r, sorted copy as float4
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_grid_count(const float *__restrict__ xyz, int P, float inv, unsigned nb,
                                                    int *__restrict__ cnt, unsigned *__restrict__ bkt,
                                                    unsigned long long *__restrict__ cellk)
{
    for (int j = blockIdx.x * 256 + threadIdx.x; j < P; j += gridDim.x * 256) {
        const int cx = scene_cell(xyz[3 * j], inv), cy = scene_cell(xyz[3 * j + 1], inv),
                  cz = scene_cell(xyz[3 * j + 2], inv);
        const unsigned b = mod_mul(bp_hash3(cx, cy, cz), nb);
        bkt[j] = b;
        cellk[j] = pack3(cx, cy, cz);
        atomicAdd(&cnt[b], 1);
    }
}

// cnt returns to zero (ready for the next scene)
__global__ __launch_bounds__(256) void k_grid_scatter(const float *__restrict__ xyz, int P,
                                                      const unsigned *__restrict__ bkt,
                                                      const unsigned long long *__restrict__ cellk,
                                                      const int *__restrict__ start, int *__restrict__ cnt,
                                                      float4 *__restrict__ gpts, int *__restrict__ gidx,
                                                      unsigned long long *__restrict__ gcell)
{
    for (int j = blockIdx.x * 256 + threadIdx.x; j < P; j += gridDim.x * 256) {
        const unsigned b = bkt[j];
        const int pos = start[b] + atomicSub(&cnt[b], 1) - 1;
        // w: the scene index's bits (the query reads point and id in one 16-byte load)
        gpts[pos] = make_float4(xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2], __int_as_float(j));
        gidx[pos] = j;
        gcell[pos] = cellk[j];
    }
}

}  // namespace mc
