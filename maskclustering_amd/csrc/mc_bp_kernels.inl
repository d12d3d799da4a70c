// mc_bp_kernels.inl — S1 mask back-projection for gfx950 (utils/mask_backprojection.py:70-151 with
// utils/geometry.py:9-24); included by mc_api.hip after mc_kernels.inl, whose mc_dev_common.inl
// (wave and block helpers, sync_global) and mc_scan.inl (the device scans) these kernels use.  The kernels
// live in one file per step of bp_run (the includes below); this file holds what they all see.
//
// The Open3D / pytorch3d semantics restated here are those of oracle/s1_oracle.c, whose header lists
// the choices (u1)-(u4) made where the libraries' result is not determined by their algorithm.  The
// kernels implement the same arithmetic: built with -ffp-contract=off, so every double operation is
// rounded where the oracle rounds it; the one FMA the CUDA ball query has is written out.
//
// Once per scene (bp_build_grid, mc_bp_grid.inl):
//   k_grid_count, scan, k_grid_scatter   the scene points bucketed by cells of 2r, a sorted copy
// One launch sequence per batch of frames, group by group as mc_bp_host.inl's bp_launch_* functions issue
// it; every data-dependent count is read on the device:
//  bp_launch_pixels (mc_bp_pixels.inl; k_bp_stat_init: mc_bp_batch.inl)
//   k_bp_stat_init                 the batch's status block: error frame, counters and tickets
//   k_bp_count     (band, frame)   per-id valid-pixel counts, id presence, depth == trunc, inf pose
//   k_bp_frames    (frame)         per-id totals -> per-band offsets; candidate masks; error status
//   scan                           candidate slots (frames, then ids ascending) and their pixel ranges
//   k_bp_slots                     slot table
//   k_bp_compact   (band, frame)   stable row-major pixel list of every slot
//  bp_launch_voxel (mc_bp_voxel.inl)
//   k_bp_vox_order one WG          slots largest first, by pixel count
//   k_bp_voxel_lds<256, 2176, 2048, 0, 5>   WG per slot, every slot: voxel_down_sample with the voxel hash
//                                  in LDS: sums in pixel order, first-occurrence voxel order
//   k_bp_voxel_lds<512, 12288, 8192, 512>   the slots the first tier listed (more voxels, a wider span)
//   k_bp_voxel     WG per slot     the slots the second tier listed: the hash in global memory
//  bp_launch_denoise (mc_bp_denoise_common.inl, mc_bp_denoise_lds.inl, mc_bp_denoise.inl)
//   k_bp_vox_order one WG          slots largest first, by voxel count (the denoise's and the query's order)
//   k_bp_classify                  a list of slots per size class
//   side stream:   k_bp_denoise_lds<16384>, then k_bp_denoise (slots of more than kBpLdsN voxels)
//   class streams: k_bp_denoise_lds<3072>, <4096>, <2048>, <1024>, <512>, each on a stream of its own
//                  WG per slot (tickets): DBSCAN + 20 % class filter + the k-NN means of the statistical
//                                  outlier removal; k_bp_denoise also the statistics + f32 AABB
//   (the streams join)
//   k_bp_knn_ring<4>  thread per point   the k-NN means the LDS classes deferred
//   k_bp_denoise_tail wave per slot      the LDS classes' outlier statistics, survivors and f32 AABB
//  bp_launch_query (mc_bp_query.inl)
//   k_bp_query_lds WG per slot     ball query (first K by scene index) over the slot's cropped scene points,
//                                  cell-sorted in LDS; coverage, the set; large slots -> a list for
//   k_bp_query<1, 20> or <1, 32>   WG per slot: the same query walking the hashed scene grid per mask point
//   scan                           kept masks' indices and offsets
//  bp_emit_pack (mc_bp_batch.inl), after the host has read the status block
//   k_bp_emit      wave per slot   kept masks -> CSR (frame column, id, sorted unique scene ids)
//   k_bp_pack                      the batch's masks and per-slot statistics in one readback buffer
// Every per-slot array lives in the slot's pixel range [pix, pix + npix) (npix bounds every per-slot
// count), so no allocation depends on a device result.
#include "mc_internal.hpp"
#include "mc_bp_knnsel.hpp"
#include "mc_bp_qcell.hpp"
#include "mc_bp_ring.hpp"
#include "mc_bp_world.hpp"

#include <cfloat>

namespace mc {

constexpr int kBpBand = 16;        // image rows per (band, frame) block
constexpr int kBpKnnMax = 20;      // sor_neighbors <= 20 (geometry.py:22 uses 20)
constexpr int kBpBallMax = 32;     // ball_k <= 32
constexpr int kBpStage = 2048;     // LDS staging of the outlier statistics
constexpr unsigned long long kEmptyKey = ~0ull;

struct BpDev {
    double trunc, vs, eps2, ce, frac, std_ratio, cov;
    double rvs;        // RN(1 / vs): the voxel index by div_rn
    double knn_r2[3];  // k-NN pre-selection radii^2 (0.6, 0.75, 0.9 eps): the 16384 class's 2-bit entry classes
    double knn_s;      // 16 / eps2: the scale of the 16 distance classes (mc_bp_knnsel.hpp), classes <= 4096
    float r2, scene_inv;
    int minpts, knn, kball, few;
    int H, W, nbands;
    int nbcap;  // eps lists read only for counts <= nbcap (<= kBpNbCap; smaller: a test knob for the cell-walk paths)
    int vec4;  // W % 4 == 0 with a 16-byte aligned depth and a 4-byte aligned seg pointer: 4 pixels per lane
};

}  // namespace mc

// In dependency order.  It is also the kernels' order in the code object (what scripts/kernel_resources.py
// lists): a file moved up or down here moves its kernels there.
#include "mc_bp_common.inl"          // stamps, hashes and keys, ordered insert, reductions
#include "mc_bp_grid.inl"            // per scene: the hashed scene grid
#include "mc_bp_pixels.inl"          // bp_launch_pixels
#include "mc_bp_voxel.inl"           // bp_launch_voxel
#include "mc_bp_denoise_common.inl"  // bp_launch_denoise: helpers of every denoise kernel
#include "mc_bp_denoise_lds.inl"     //   size classes, k_bp_classify, k_bp_denoise_lds (includes mc_bp_dbg.inl)
#include "mc_bp_denoise.inl"         //   k_bp_knn_ring, k_bp_denoise_tail, k_bp_denoise
#include "mc_bp_query.inl"           // bp_launch_query
#include "mc_bp_batch.inl"           // k_bp_stat_init, k_bp_emit, k_bp_pack
