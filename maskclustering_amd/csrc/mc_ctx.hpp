// mc_ctx.hpp — the context of libmcgraph: struct mc_ctx and one state struct per stage that owns state
// (included by mc_api.hip, same translation unit, before the entry points and the host drivers).
// A field belongs to the stage that writes it; a later stage reaches it through its owner's name
// (ctx->cluster.d_final_label inside mc_pp_run_clustered), so a call site shows whose buffer it reads.
namespace {

// device-side statistics block (copied to pinned host memory in one transfer)
enum Stat : int {
    ST_NBND = 0,      // boundary points
    ST_NNZC = 1,      // contained entries after undo
    ST_N0 = 2,        // level-0 nodes
    ST_NTHR = 3,      // thresholds
    ST_THR_STATUS = 4,
    ST_K = 5,         // final objects
    ST_WORDS = 6,     // point-bitmap words
    ST_NPTS = 7,      // object points (sum)
    ST_OBJOVF = 8,    // a point in more objects than the per-point fast path holds
    ST_COUNT = 9,
};

// the arrays of one S6 level (device pointers): per node the offset and length of its row of
// contained masks in `pool`, the owner node of every pool entry, the nodes' visible-frame words
struct S6Level {
    int *off = nullptr, *len = nullptr, *pool = nullptr, *own = nullptr;
    unsigned long long *vf = nullptr;
};

// S1 back-projection state of a context (the host code is mc_bp_host.inl)
struct BpState {
    // scene points and their 2r grid
    int64_t P = 0;
    bool have_points = false, have_result = false;
    float grid_radius = -1.f;  // scene grid built for this ball radius
    unsigned gnb = 0;
    DevBuf scene, gcnt, gstart, gbkt, gcellk, gpts, gidx, gcell, gscan_tmp;
    // frames that arrive from the host
    DevBuf in_depth, in_seg, in_intr, in_pose, in_raw;
    char *h_stage[2] = {nullptr, nullptr};  // pinned staging ring of mc_backproject_frames (two chunks, ping-pong)
    size_t stage_bytes = 0;
    hipEvent_t ev_stage[2] = {};
    bool stage_used[2] = {false, false};
    hipStream_t copy = nullptr;  // host frames staged batch by batch while the previous batch computes
    hipEvent_t ev_up = nullptr;
    // per-batch arrays
    DevBuf band, present, fflags, cand, npix, csidx, poff, slot_of, stat;
    DevBuf vid;  // valid-id map (k_bp_count -> k_bp_compact), 1 byte per pixel
    DevBuf slot_frame, slot_id, slot_np, slot_pix, slot_nv, slot_m, slot_ns, slot_box, slot_nn, slot_toff, slot_cov;
    DevBuf pix_list, hkey, hvid, hfirst, vox_entry, acc, vpts, pcell, pbkt, bcnt, bstart, blist, ncnt, par, droot, rnk,
        lab, ccnt, ssidx, avg, qpts;
    DevBuf bm, tmp, kflag, ksize, midx, moff, out_col, out_label, out_off;
    DevBuf cls_list, nbl, lean, vox_order;  // denoise size-class slot lists; per-workgroup eps-neighbour lists, lean scratch
    DevBuf vx_pvid, vx_list, vx_fb;  // voxel_down_sample: per-pixel voxel ids and voxel lists of k_bp_voxel_lds; its overflow slots
    DevBuf q_fb;       // ball query: the slots k_bp_query_lds hands to k_bp_query
    DevBuf scanm;      // block sums of the multi-workgroup scans
    DevBuf slot_grid;  // denoise: grid origin / extent of the slots with points queued for the k-NN ring search
    DevBuf pack;       // the batch's readback, packed (k_bp_pack)
    int *h_pack = nullptr;  // its pinned copy, h_pack_n ints
    size_t h_pack_n = 0;
    hipEvent_t ev_pack = nullptr;  // the last batch's h_pack copy (appended under the next batch)
    int *h_stat = nullptr;         // pinned copy of the status block
    hipStream_t cls_stream[mc::kBpStreamClasses] = {};  // denoise: the LDS size classes run side by side
    hipEvent_t ev_cls[mc::kBpStreamClasses] = {};
    // batch sizing
    int64_t mem_budget = 0;  // bytes the per-batch arrays may take (0: the default share, mc_bp_plan.hpp)
    size_t px_cap = 0;       // mask-pixel capacity of the per-batch arrays (pixel-list positions)
    size_t fpx_cap = 0;      // frame-pixel capacity (the valid-id map)
    double mfrac = 1.0;      // mask pixels per frame pixel a batch is sized for (the largest seen, + margin)
    bool mfrac_obs = false;  // mfrac comes from an earlier call's batches (not the initial guess)
    int last_fb = 0;         // frames per batch at the end of the last call
    int64_t redo = 0;        // batches redone after a mask-pixel overflow (all calls)
    // results of the last call
    int F = 0, err_frame = -1;
    int64_t nnz = 0;
    DevBuf pts;  // the masks' point lists
    std::vector<int32_t> col, label, stats;
    std::vector<int64_t> off;
    // the voxel stage's read-back (mc_backproject_get_voxels): the batches the last call accepted (the per-batch
    // arrays hold the last one's slots), and the slots the accepted batch's voxel tiers handed on
    int batches = 0;
    int vx_handed[2] = {0, 0};
};

// AP evaluation state of a context (the host code is mc_ap_host.inl; EvTables is mc_ap_plan.hpp's)
struct EvState {
    bool active = false;
    int C = 0, O = 0, nlab = 0;
    int64_t min_region = 100;
    bool no_class = false;
    std::vector<int32_t> class_ids;
    std::vector<double> overlaps;
    DevBuf d_lab2cls, d_overlaps;
    // accumulated over the scans: examples in per-unit regions, one unit per (scan, class, overlap)
    int64_t ex_used = 0;
    int units = 0;
    DevBuf d_ex_key, d_ex_true, d_unit_cell, d_unit_off, d_unit_cnt, d_hardfn, d_flags;
    EvTables last;
    bool have_last = false;
    // the table of the last mc_ev_ap
    bool ap_valid = false;
    std::vector<double> ap;
    std::vector<int64_t> stats;
    std::vector<int32_t> ndist;
    DevBuf d_key, d_true, d_prec, d_rec, d_cell, d_ap, d_stats, d_ndist;
    // the accumulation as runs (mc_ev_state_*): the state buffer of the last export, kept on the device
    bool runs_valid = false;
    int64_t state_runs = 0, state_examples = 0, state_bytes = 0;
    DevBuf d_state, d_run;
    // scratch of one call, by the step that writes it
    DevBuf d_in[5];  // mc_ev_add_scan*: the host arguments' device copies
    DevBuf d_info;   // validate (ev_scan_validate, ev_merge_check_runs): the flag words; the scan's table sizes
    // the scan tables (ev_scan_carve, ev_scan_launch, ev_scan_fetch): compact tables in d_out, fetched to h_out
    DevBuf d_cnt, d_inst, d_tmp_id, d_class, d_gcls, d_gid, d_gvert, d_pinst, d_pk, d_pair_gt, d_pair_int, d_out;
    std::vector<int64_t> h_out;
    DevBuf d_words, d_tmp;  // commit (ev_greedy_pass): the word block and the pass's temporaries; the merge's run offsets and cells
    DevBuf d_merge;         // merge (ev_merge_sections): the device copy of a host state buffer
};

// CLIP crop preparation (mc_crop_*; the host code is mc_crop_host.inl): the context's pools
struct CropState {
    DevBuf tab, frames, slot, label;          // boxes: per-frame label tables, the referenced frames, per-mask slot / label
    DevBuf in_seg, in_rgb, in_boxes, in_status, out_boxes, out_status;  // host arguments' device copies
    DevBuf mframe, lut, bounds, kk, tmp;      // render: per-mask frame, 3 x 256 table, coefficient tables, intermediate
    std::vector<int32_t> h_frames, h_slot, h_label, h_mframe;  // staged until the next call
    std::vector<float> h_lut;
};

// projected boxes (mc_proj_*; the host code is mc_proj_host.inl): the context's pools
struct ProjState {
    DevBuf pts, intr, w2c, opoff, opts;          // host arguments' device copies (pts also: the widened scene points)
    DevBuf gobj, goff, rframe, rout;             // the request groups of mc_proj_boxes
    DevBuf acc, flag, ocol;                      // accumulators, the check flag, the final objects' mask frames
    DevBuf out_pos, out_frame, out_boxes, out_status, out_inside;  // host outputs' device copies
    std::vector<int32_t> h_gobj, h_goff, h_rframe, h_rout;         // staged until the next call
};

// scene point cloud fusion (mc_cloud_*; the host code is mc_cloud_host.inl): the result of the last call
struct CloudState {
    bool have = false, have_col = false;
    int64_t n = 0;                                // result points
    DevBuf pts, col;                              // float64 [n, 3] each
    int64_t stages = 0, max_in = 0, max_pop = 0;  // voxel_down_sample runs, the largest one's input, the fullest voxel
};

// label painter (mc_labels_paint; the host code is mc_paint_host.inl): the context's pools
struct PaintState {
    DevBuf planes, stage;                      // a round's bit planes; its masks when they come from the host
    DevBuf off, scores, area, order;           // instance offsets, scores (host input), areas, kept lists in paint order
    DevBuf kept, status, labinst;              // per frame: kept count, status; the id -> instance table of a host output
    std::vector<int64_t> h_off;                // staged until the next call
};

// scene input (mc_scene_set_masks; the host code is mc_graph_host.inl): the kept masks on the host and the device
// (P, F and FW are also set by mc_nodes_set, which brings level-0 nodes without a scene)
struct SceneState {
    bool have = false;
    int64_t P = 0;
    int F = 0, FW = 0, M = 0, M_in = 0;
    int nnz = 0;
    std::vector<int32_t> h_col, h_label, h_in_index, h_off;
    DevBuf d_mask_off, d_mask_pts, d_mask_col, d_mask_label, d_frame_start, d_valid;
};

// S2–S5 and the level-0 nodes (mc_graph_build, mc_nodes_set; the host code is mc_graph_host.inl)
struct GraphState {
    bool have = false, have_nodes = false;
    bool nodes_from_graph = false;
    // ---- S2 ----
    DevBuf d_deg, d_pt_off, d_pt_list, d_boundary, d_pfm, d_scan_tmp;
    DevBuf d_spread;  // spread slots of the S2 boundary counter
    // ---- S3/S5 ----
    DevBuf d_ctmp, d_crow_len, d_useg, d_keep_cnt, d_node_flag, d_node_pos, d_c_off, d_c_idx, d_vf;
    DevBuf d_s3_small, d_s3_big;
    int n_s3_small = 0, n_s3_big = 0;
    // ---- S4 ---- (d_thr: mc_cluster_run writes the caller's thresholds there when it is given any)
    DevBuf d_hist, d_thr, d_isint, d_s4rng;
    // ---- level-0 nodes ----
    int N0 = 0;        // host copy (valid after sync_stats or mc_nodes_set)
    int Mn = 0;        // mask-id space of C rows
    int64_t n0_pts_total = 0;
    DevBuf d_node0_g, d_n0_off, d_n0_len, d_n0_ptoff, d_n0_ptlen, d_n0_vf, d_user_cidx, d_user_pts;
    DevBuf d_owner0, d_node_of_mask;
    int *n0_pool = nullptr;
    const int *n0_pts = nullptr;
    int64_t nnzC0 = 0;
};

// S6 iterative clustering and S7 final point sets (mc_cluster_*; the host code is mc_cluster_host.inl)
struct ClusterState {
    bool have = false;
    // the run's mode, kept across the FOREST exchange of a sharded context
    int nthr = 0;
    bool dense_obs = false;
    float ctf = 0.f;
    // ---- S6 ----
    DevBuf d_parent, d_root, d_isroot, d_rank, d_label, d_levels, d_memcnt, d_memoff, d_ublen, d_newoff;
    DevBuf d_members, d_colcnt, d_coloff, d_collen, d_colnodes, d_ovf_n, d_scratch, d_touched, d_edges;
    DevBuf d_Nlev, d_final_label;
    DevBuf d_poolA, d_poolB, d_offA, d_offB, d_lenA, d_lenB, d_vfA, d_vfB, d_ownA, d_ownB, d_cap;
    int scratch_n0 = -1;
    int n_iter = 0;
    S6Level fin;  // the final objects (the last level, in the pools)
    int K = 0;
    int64_t npts = 0;
    // edge capture for the set-order replay (mc_cluster_set_edge_capture)
    int64_t cap_edges = 0;
    DevBuf d_cap_buf, d_cap_cnt;
    // ---- S7 ---- (d_obj_of_mask is sized with the scene's buffers, scene_reserve)
    DevBuf d_obj_of_mask, d_pmin, d_pmax, d_nwords, d_woff, d_bm, d_ptcnt, d_ptoff_out, d_pts_out;
};

// row-block sharding over processes (mc_shard_*, mc_ctx_comm_*; the host code is mc_shard_host.inl)
struct ShardState {
    int rank = 0, world = 1;
    int pending = 0;          // MC_SHARD_* phase waiting for the host's exchange, 0 = none
    int r0 = 0, r1 = 0;       // this rank's S3 mask rows (build_s3_lists, mc_graph_host.inl)
    int64_t s3_words = -1;    // size of this rank's S3 block (valid while pending == MC_SHARD_S3)
    mc_graph_params params{};
    DevBuf d_eoff;
    // native collectives (mc_ctx_attach_comm / mc_ctx_comm_init): with a communicator attached the
    // sharded mc_graph_build / mc_cluster_run run their exchanges themselves, on the context stream
    void *comm = nullptr;        // ncclComm_t
    bool own_comm = false;
    DevBuf d_send, d_recv, d_size;
};

// post-processing and export of the clustered objects (mc_pp_*; the host code is mc_pp_host.inl)
struct PpState {
    DevBuf d_posmap;  // one P-entry position map per workgroup, -1 at rest
    int64_t posmap_P = 0;
    int posmap_slots = 0;
    bool have = false;
    mc_pp_info info{};
    std::vector<int32_t> entry_obj, qobj, obj_node;
    std::vector<double> qcov, box;
    std::vector<uint8_t> state;
    // the node arrays and per-entry results of the last run, resident for the export
    DevBuf d_npoff, d_npts, d_qoff, d_qm, d_eobj, d_qobj, d_qcov;
    DevBuf d_qcol;  // the node masks' frame columns (mc_proj_top_views)
    int64_t P = 0;
    int F = 0;
    bool host = false;         // entry_obj / qobj / qcov are fetched (mc_pp_get_results)
    bool have_export = false;  // the export arrays below are built
    std::vector<int32_t> fslot, fin, fin_node;  // object -> final slot; final objects, their nodes
    std::vector<int64_t> opoff, omoff;          // point / mask list offsets of the final objects
    DevBuf d_fslot, d_finobj, d_finnode, d_opoff, d_omoff, d_opts, d_omask, d_ocov, d_repre;
};

}  // namespace

struct mc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t side = nullptr;                 // S3: workgroup-per-mask kernel beside the wave kernel
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::string err;
    mc::KernelTimer timer;
    // the statistics block (Stat): S3, S4, S6 and S7 write it, every stage reads it
    int *h_stats = nullptr;  // pinned
    DevBuf d_stats;
    int num_cu = 256;
    int max_lds = 64 * 1024;  // LDS one workgroup may ask for (hipDeviceAttributeMaxSharedMemoryPerBlock)

    BpState bp;            // S1 back-projection (mc_bp_*)
    SceneState scene;      // the scene's masks (mc_scene_set_masks)
    GraphState graph;      // S2–S5, level-0 nodes (mc_graph_*, mc_nodes_set)
    ClusterState cluster;  // S6, S7 (mc_cluster_*)
    ShardState shard;      // row-block sharding over processes (mc_shard_*)
    PpState pp;            // post-processing and export (mc_pp_*)
    EvState ev;            // AP evaluation (mc_ev_*)
    CropState crop;        // CLIP crop preparation (mc_crop_*)
    ProjState proj;        // projected boxes (mc_proj_*)
    CloudState cloud;      // scene point cloud fusion (mc_cloud_*)
    PaintState paint;      // label painter (mc_labels_paint)
};
