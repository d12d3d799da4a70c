// mc_pp_kernels.inl — post-processing of the clustered objects on gfx950; included by
// mc_api.hip after mc_bp_kernels.inl, whose cell hash, keys and reductions (mc_bp_common.inl) and shell walk
// these kernels use.  The kernels live in one file per step of mc_pp_host.inl's driver (the includes below);
// this file holds what they all see.
//
// The reference's utils/post_process.py:173-195 per scene:
//   dbscan_process (:104-123)   Open3D DBSCAN(eps 0.1, min 4) of each node's points, one object per
//                               label class (class 0 = noise), in list(node.point_ids) order;
//   filter_point (:40-101)      per object point: frames of the node where it is seen (pfm) and where
//                               a mask of the node holds it; the detection-ratio filter; every node mask
//                               assigned to the object it intersects most (coverage = |m ∩ o| / |o|);
//   merge_overlapping_objects   greedy i < j pass over all kept objects with the bbox test
//   (:7-37)                     (utils/geometry.py:3-7) and the 0.8 intersection ratios.
//
// Layout: the nodes' points are one entry array (node k owns entries [pt_off[k], pt_off[k+1]) in
// its list order); every per-entry scratch array is indexed by entry, so nodes never share scratch.
// k_pp_dbscan and k_pp_filter are persistent workgroups taking nodes largest-first from a ticket.
//
//   file               kernels                                                      launched by
//   mc_pp_dbscan.inl   k_pp_gather, k_pp_dbscan<512>, k_pp_big_grid<512>,           pp_dbscan
//                      k_pp_big_walk<512, 0 / 1>, k_pp_big_label<512>
//   mc_pp_filter.inl   k_pp_filter                                                  pp_filter
//   mc_pp_merge.inl    k_pp_index, k_pp_pairs, k_pp_decide, k_pp_greedy             pp_merge
//   mc_pp_layout.inl   k_pp_validate, k_pp_prep, k_pp_order, k_pp_scan64            pp_layout
//                      k_pp_widen, k_pp_cl_count / keep / select / masklen /        mc_pp_run_clustered (and
//                      members / gather                                             k_pp_scan64 again)
//   mc_pp_export.inl   k_pp_ex_fill, k_pp_ex_repre                                  pp_build_export
//                      k_pp_ex_pred                                                 mc_pp_export_pred_masks

namespace mc {

// The sizes the host (mc_pp_host.inl) and the tests (tests/pp_limit_inputs.py reads them out of this file) name:
constexpr int kPPObjChunk = 1024;  // k_pp_filter: per-wave LDS counters of mask ∩ object
constexpr int kPPBoxChunk = 256;   // k_pp_filter: per-workgroup LDS bbox / kept-point accumulators
constexpr int kPPSlots = 16;       // pp_merge: objects per point in the intersection index (grown on demand)
constexpr int kPPLdsUF = 8192;     // k_pp_dbscan: nodes up to this many points keep their union-find in LDS
// k_pp_prep: a node's extent along an axis, in DBSCAN cells, stays below this (pack3 keeps 21 bits per axis)
constexpr double kPPMaxCells = static_cast<double>((1 << 21) - 1);

struct PPDev {
    double eps2, ce, thr, ratio;
    int minpts;
};

// order-preserving map of a double onto u64 (no NaNs on this path): min/max by integer atomics
__device__ __forceinline__ unsigned long long pp_ord(double v)
{
    const unsigned long long u = __double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double pp_unord(unsigned long long u)
{
    return __longlong_as_double((u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u);
}

// block min / max of 3 doubles over NT threads, broadcast; red holds 6 * NT/64 doubles (pp_grid, k_pp_prep).
// Not one template with block_minmax3 of mc_bp_common.inl: beside the barrier, that one folds its four
// partials pairwise and this one serially, so either text in the other's place changes the instructions of
// k_bp_voxel and k_bp_denoise, or of k_pp_prep (tried: docs/experiments.md, "Post-processing kernel files").
template <int NT>
__device__ __forceinline__ void pp_block_minmax3(double mn[3], double mx[3], double *red)
{
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double lo = wave_min_d(mn[c]), hi = wave_max_d(mx[c]);
        if (lane == 0) {
            red[c * NW + wv] = lo;
            red[(3 + c) * NW + wv] = hi;
        }
    }
    sync_global();
#pragma unroll
    for (int c = 0; c < 3; c++) {
        mn[c] = red[c * NW];
        mx[c] = red[(3 + c) * NW];
        for (int w = 1; w < NW; w++) {
            mn[c] = fmin(mn[c], red[c * NW + w]);
            mx[c] = fmax(mx[c], red[(3 + c) * NW + w]);
        }
    }
    sync_global();
}

}  // namespace mc

// In the kernels' order in the code object (what scripts/kernel_resources.py lists): a file moved up or down
// here moves its kernels there.
#include "mc_pp_dbscan.inl"  // pp_dbscan: dbscan_process, a node per workgroup or split over the chip
#include "mc_pp_filter.inl"  // pp_filter: filter_point
#include "mc_pp_merge.inl"   // pp_merge: merge_overlapping_objects
#include "mc_pp_layout.inl"  // pp_layout: argument checks, per-node layout; the clustered entry's node arrays
#include "mc_pp_export.inl"  // the export of the final objects
