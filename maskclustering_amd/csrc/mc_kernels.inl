// mc_kernels.inl — gfx950 kernels of the view-consensus graph path, S2 to S7 (included by mc_api.hip), and
// the device helpers and scans that every other kernel file of the library uses.  The kernels live in one
// file per stage (the includes below); this file holds the layout they share and says where things are.
//
// Data layout in HBM:
//   mask CSR      mask_off[M+1] (i32), mask_pts[nnz] (i32)      S1 output, read-only
//   point lists   pt_off[P+1], pt_list[nnz] (u32 = frame<<12 | mask-in-frame), sorted per point
//   boundary[P]   u8;  pfm[P][FW] u64 point-frame bits (FW = ceil(F/64))
//   C rows        c_off[M+1], c_idx[nnzC] (global mask ids, ascending) — contained_masks after undo
//   VF            vf[M][FW] u64 — visible_frames after undo (== frames of the C row)
//   nodes (S6)    (off,len) into a C pool + slot owner per pool slot + vf[N][FW]; pools ping-pong
//
// Every kernel that works on a data-dependent count reads it from device memory
// (no host round trip inside the S6 loop).  Counters that kernels accumulate into
// are restored to zero by the kernel that consumes them (no per-iteration memsets).
//
// File, its kernels (and the constants and structs the host names), the host step that launches them
// (graph_* and launch_hist: mc_graph_host.inl; s6_* and s7_*: mc_cluster_host.inl):
//   mc_dev_common.inl   wave_sync, sync_global, wave_incl_scan / _sum / _min_i / _max_i, block_excl_scan,
//                       block_sum, ld_agent, st_agent, lane_id, spread_add; kSpread, kSpreadStrideI,
//                       kSpreadStrideL                                      every kernel file (S1, post-
//                                                                           processing, shard, projection, AP, ...)
//   mc_scan.inl         k_scan1, k_scan_reduce, k_scan_down, k_scanm_reduce, k_scanm_down; ScanArrays
//                                                                           scan_device_n, scan_device_multi,
//                                                                           scan_large (here), from every stage
//   mc_s2_kernels.inl   k_s2_degree, k_s2_scatter, k_s2_points              graph_s2_point_lists
//                       k_s2_dense_pim                                      mc_graph_get_point_in_mask
//   mc_s3_kernels.inl   k_s3_masks<W>; S3Cfg, MC_S3_BIGW / _SMALL / _BATCH / _U / _REP, kS3BigW, kS3SmallPts,
//                       kS3wCounters, kS3wFrameWords64                      graph_s3_masks
//                       k_s3_undo_count, k_s3_undo_write, k_s5_nodes        graph_undo_s5_hist
//   mc_s4_kernels.inl   k_s4_ranges, k_s4_hist                              launch_hist
//                       k_s4_thresholds                                     graph_thresholds, mc_observer_thresholds
//   mc_s6_columns.inl   uf_find, uf_unite; k6_colcount, k6_colscatter, k6_colupdate    s6_level0_columns
//                       k6_parent_init                                      s6_pairs_dense
//                       col_update_block, ColUpdate                         (inside k6_merge's launch)
//   mc_s6_pairs.inl     k6_pairs; EdgeRule, EdgeCap, OvfWork, kOvfSlots, kPairWaves, MC_ABLATE_PAIRS    s6_pairs
//                       k6_pairs_dense                                      s6_pairs_dense
//   mc_s6_merge.inl     k6_compress, k6_relabel, k6_memscatter, k6_components    s6_components
//                       k6_merge                                            s6_merge
//                       k6_init                                             s6_init
//   mc_s7_kernels.inl   k7_reset, k7_obj_of_mask, k7_minmax, k7_words, k7p_points<0>    s7_ranges
//                       k7p_points<1>, k7_setbits, k7_count, k7_extract     s7_points
//                       k_copy_i32                                          (no launcher)
#include "mc_internal.hpp"

#include <climits>

// In dependency order.  It is also the kernels' order in the code object (what scripts/kernel_resources.py
// lists): a file moved up or down here moves its kernels there.
#include "mc_dev_common.inl"
#include "mc_scan.inl"
#include "mc_s2_kernels.inl"
#include "mc_s3_kernels.inl"
#include "mc_s4_kernels.inl"
#include "mc_s6_columns.inl"
#include "mc_s6_pairs.inl"
#include "mc_s6_merge.inl"
#include "mc_s7_kernels.inl"
