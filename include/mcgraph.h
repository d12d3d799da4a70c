/*
 * mcgraph.h — C-ABI of the MI355X-native view-consensus graph path of
 * MaskClustering (libmcgraph.so, hand-written HIP kernels for gfx950).
 *
 * The library replaces the compute behind these reference interfaces
 * (paths relative to the reference repository):
 *
 *   graph/construction.py:7    mask_graph_construction      -> mc_scene_set_masks + mc_graph_build
 *   graph/construction.py:22   build_point_in_mask_matrix   -> mc_graph_build (S2)
 *   graph/construction.py:137  process_masks / :98 process_one_mask -> mc_graph_build (S3)
 *   graph/construction.py:80   get_observer_num_thresholds  -> mc_graph_build (S4) + mc_graph_get_thresholds
 *   graph/construction.py:66   init_nodes                   -> mc_graph_build (S5)
 *   graph/iterative_clustering.py:36 iterative_clustering   -> mc_cluster_run
 *   graph/iterative_clustering.py:13 update_graph           -> mc_cluster_run (pair counts + edge rule)
 *   graph/iterative_clustering.py:5  cluster_into_new_nodes -> mc_cluster_run (components)
 *   graph/node.py:24           Node.create_node_from_list   -> mc_cluster_run (on-device merge)
 *   utils/mask_backprojection.py:70 turn_mask_to_point      -> mc_backproject (S1)
 *   utils/mask_backprojection.py:154 frame_backprojection   -> mc_backproject + mc_backproject_get_masks
 *   utils/geometry.py:9        denoise                      -> mc_backproject (S1 denoise)
 *
 * Conventions
 *   - Every call returns 0 (MC_OK) or an MC_ERR_* code; mc_ctx_last_error()
 *     gives the message.  No call throws.
 *   - Host buffers are caller-owned; sizes are given by the *_get_info calls
 *     (two-call pattern: query sizes, then fill).
 *   - The context owns all device memory.  One context per device per host
 *     thread; no global state.  Work is enqueued on the context's HIP stream
 *     (its own, or the one given by mc_ctx_set_stream); getters synchronise it.
 *   - Masks are the reference's per-frame mask dicts flattened in frame
 *     order, ids in dict order (construction.py:46-60); frames whose mask
 *     union is empty are dropped like construction.py:50-51.
 */
#ifndef MCGRAPH_H
#define MCGRAPH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MC_OK 0
#define MC_ERR_INVALID 1          /* bad argument / inconsistent input            */
#define MC_ERR_HIP 2              /* HIP runtime error                            */
#define MC_ERR_STATE 3            /* call out of order (e.g. cluster before build)*/
#define MC_ERR_EMPTY_OBSERVERS 4  /* np.percentile on empty (construction.py:89)   */
#define MC_ERR_UNSUPPORTED 5      /* size beyond a documented limit                */
#define MC_ERR_NO_NODES 6         /* torch.stack([]) (iterative_clustering.py:17)  */

typedef struct mc_ctx mc_ctx;

/* args fields read by graph/construction.py:119,125,132 */
typedef struct {
    double mask_visible_threshold;
    double contained_threshold;
    double undersegment_filter_threshold;
} mc_graph_params;

typedef struct {
    int64_t num_points;        /* P                                   */
    int32_t num_frames;        /* F (columns of the frame list)       */
    int32_t num_masks;         /* M: global masks (kept)              */
    int32_t num_undersegment;  /* |U|                                 */
    int32_t num_nodes0;        /* N0 = M - |U|                        */
    int64_t num_contained;     /* nnz of contained_masks after undo   */
    int64_t num_boundary;      /* |boundary_points|                   */
    int32_t num_thresholds;    /* len(observer_num_thresholds)        */
    int32_t threshold_status;  /* MC_OK or MC_ERR_EMPTY_OBSERVERS     */
} mc_graph_info;

typedef struct {
    int32_t num_iterations;    /* thresholds consumed                 */
    int32_t num_objects;       /* final nodes                         */
    int32_t num_nodes0;        /* nodes entering iteration 0          */
    int32_t reserved;
    int64_t num_object_points; /* sum over objects of |point_ids|     */
    int64_t num_object_contained; /* sum over objects of |contained|  */
    int64_t num_object_masks;  /* sum over objects of |mask_list|     */
} mc_cluster_info;

/* S1 constants (utils/mask_backprojection.py:8-14,38; utils/geometry.py:10,16,22).
 * Same layout as the oracle's orc_bp_params.  mc_bp_params_default() fills
 * the reference's values. */
typedef struct {
    double depth_trunc;            /* DEPTH_TRUNC = 20                      */
    double voxel_size;             /* DISTANCE_THRESHOLD = 0.01 (voxel)     */
    double dbscan_eps;             /* 0.04                                  */
    double component_min_fraction; /* 0.2                                   */
    double sor_std_ratio;          /* 2.0                                   */
    double ball_radius;            /* DISTANCE_THRESHOLD (as float32)       */
    double coverage_threshold;     /* COVERAGE_THRESHOLD = 0.3              */
    int32_t dbscan_min_points;     /* 4                                     */
    int32_t sor_neighbors;         /* 20 (<= 20)                            */
    int32_t ball_k;                /* K = 20 (<= 32)                        */
    int32_t few_points;            /* FEW_POINTS_THRESHOLD = 25             */
} mc_bp_params;

typedef struct {
    int32_t num_frames;
    int32_t num_candidates;        /* (frame, id) with >= few_points pixels  */
    int32_t num_masks;             /* kept masks (coverage >= threshold)     */
    int32_t error_frame;           /* -1, or the first frame that raises     */
    int64_t num_mask_points;       /* sum of the kept masks' set sizes       */
} mc_bp_info;

#define MC_BP_NSTAT 10  /* per candidate: frame, id, pixels, voxels, after DBSCAN filter,
                           after outlier removal, -1, covered, neighbours, kept */

/* ---- context ------------------------------------------------------------ */
int mc_ctx_create(int device, mc_ctx **out);
void mc_ctx_destroy(mc_ctx *ctx);
int mc_ctx_set_stream(mc_ctx *ctx, void *hip_stream);   /* NULL = own stream */
void *mc_ctx_get_stream(mc_ctx *ctx);
int mc_ctx_synchronize(mc_ctx *ctx);
const char *mc_ctx_last_error(mc_ctx *ctx);
/* live per-kernel timing with HIP events on the context stream (bench/profiling) */
int mc_ctx_set_timing(mc_ctx *ctx, int enable);
int mc_ctx_set_timing_filter(mc_ctx *ctx, const char *kernel);  /* NULL/"" = every kernel group */
int mc_ctx_get_kernel_time(mc_ctx *ctx, const char *kernel, double *total_ms, int64_t *launches);
int mc_ctx_reset_kernel_times(mc_ctx *ctx);
/* HBM the back-projection's per-batch arrays may take (bytes; 0 = the default: 40 % of the device
   or 65 % of the free memory, whichever is less).  Batches are sized from it (~224 B per pixel);
   a caller sharing the device with its own allocator (or other contexts) keeps the rest. */
int mc_ctx_set_memory_budget(mc_ctx *ctx, int64_t bytes);
/* diagnostics: out[0] = 1 if the library was built with in-kernel invariant checks
   (-DMC_DBG_CHECK=1), out[1 + k] = failures of check kind k so far; n <= 9 */
int mc_debug_counters(mc_ctx *ctx, int64_t *out, int32_t n, int reset);

/* ---- scene input (the S1 output: per-frame mask point sets) ---------------
 * mask_col/label/off are host arrays of length M_in, M_in, M_in+1.
 * mask_pts (length mask_off[M_in]) is a host pointer, or a device pointer
 * when pts_on_device != 0.  Point ids in [0, P); each mask's ids unique;
 * labels in [1, 65535] and unique within a frame; mask_col non-decreasing.  */
int mc_scene_set_masks(mc_ctx *ctx, int64_t num_points, int32_t num_frames, int32_t num_masks_in,
                       const int32_t *mask_col, const int32_t *mask_label, const int64_t *mask_off,
                       const int32_t *mask_pts, int pts_on_device);

/* ---- S1: per-frame mask back-projection ---------------------------------
 * utils/mask_backprojection.py:70-151 (turn_mask_to_point) for a batch of
 * frames: build_point_in_mask_matrix's per-frame loop (construction.py:46-49)
 * without the host round trips.  Scene points: float32 [P,3] (the reference
 * casts to float32 at construction.py:37).  depth float32 [F,H,W] metres,
 * seg uint8 [F,H,W] aligned with depth, intrinsics [F,4] = fx, fy, cx, cy,
 * poses [F,16] row-major camera-to-world; host pointers, or device pointers
 * when on_device != 0.  A frame with an inf pose yields no masks (:73-74); a
 * depth pixel equal to depth_trunc in a frame with mask ids fails the call
 * with MC_ERR_INVALID (the reference raises IndexError at :100).          */
void mc_bp_params_default(mc_bp_params *p);
int mc_scene_set_points(mc_ctx *ctx, int64_t num_points, const float *xyz, int on_device);
int mc_backproject(mc_ctx *ctx, int32_t num_frames, int32_t height, int32_t width, const float *depth,
                   const uint8_t *seg, const double *intrinsics, const double *poses, int on_device,
                   const mc_bp_params *params);
/* the same, with one host pointer per frame (depth_frames[f]: float32 [H,W], seg_frames[f]: uint8
 * [H,W]) as a dataset hands them out (dataset/scannet.py:48-64, construction.py:47-48): the frames
 * are staged through pinned memory by host threads while the previous chunk's DMA runs, with no
 * [F,H,W] host copy.  intrinsics / poses as above (host).                                        */
int mc_backproject_frames(mc_ctx *ctx, int32_t num_frames, int32_t height, int32_t width,
                          const float *const *depth_frames, const uint8_t *const *seg_frames,
                          const double *intrinsics, const double *poses, const mc_bp_params *params);
/* the same from the depth PNGs' raw values (depth_frames[f]: uint16 [H,W]; dataset/scannet.py:51-53,
 * scannetpp.py:168-170, matterport.py:91-93): staged as 2 bytes per pixel instead of 4 and decoded on
 * the device to float32(uint16 / depth_scale) computed in float64 -- the array get_depth returns.  */
int mc_backproject_frames_raw(mc_ctx *ctx, int32_t num_frames, int32_t height, int32_t width,
                              const uint16_t *const *depth_frames, double depth_scale,
                              const uint8_t *const *seg_frames, const double *intrinsics, const double *poses,
                              const mc_bp_params *params);
int mc_backproject_get_info(mc_ctx *ctx, mc_bp_info *info);
/* S1's batching (no reference counterpart; the library's HBM budget, mc_ctx_set_memory_budget):
 * out4 = {frames per batch at the end of the last call, mask-pixel capacity of the per-batch
 * arrays, bytes those arrays hold, batches redone after a mask-pixel overflow (all calls)}       */
int mc_backproject_get_batching(mc_ctx *ctx, int64_t *out4);
/* kept masks in frame order then id order: mask_col (frame index), mask_label
 * (id), mask_off [M+1], mask_pts = sorted unique scene ids (mask_info[id], :148) */
int mc_backproject_get_masks(mc_ctx *ctx, int32_t *mask_col, int32_t *mask_label, int64_t *mask_off,
                             int32_t *mask_pts);
int mc_backproject_get_candidates(mc_ctx *ctx, int32_t *stats /* num_candidates * MC_BP_NSTAT */);
/* test read-back of S1's pixel lists and voxel means (no reference counterpart), of a call whose frames
 * ran as exactly one batch (the arrays are per batch; otherwise, or after no call, MC_ERR_STATE).  Call
 * once with sizes3 alone, then with the arrays (any of them may be NULL):
 *   sizes3  = {slots (= num_candidates, in that order), their pixels in all, their voxels in all}
 *   slots   [slots * 4]    frame, id, pixel count, voxel count
 *   pixels  [pixels]       slot after slot, each slot's valid pixels v * width + u in list order
 *   means   [voxels * 3]   slot after slot, each slot's voxel means in voxel order
 *   origins [slots * 3]    each slot's voxel grid origin (min bound - voxel_size / 2)
 *   handed2 = {slots the first voxel tier handed to the second, slots the second handed to the global hash} */
int mc_backproject_get_voxels(mc_ctx *ctx, int64_t *sizes3, int32_t *slots, uint32_t *pixels, double *means,
                              double *origins, int32_t *handed2);
/* mask_pts into a device buffer (stream-ordered on the context stream, no host copy): the
 * frame-sharded path all-gathers the per-rank point lists over RCCL;
 * mask_col / mask_label / mask_off come from mc_backproject_get_masks with mask_pts = NULL */
int mc_backproject_copy_points_device(mc_ctx *ctx, int32_t *mask_pts_dev);

/* the back-projected masks become the graph input (as mc_scene_set_masks, device-resident) */
int mc_scene_use_backprojection(mc_ctx *ctx);

/* ---- S2-S5: graph construction ------------------------------------------ */
int mc_graph_build(mc_ctx *ctx, const mc_graph_params *params);
int mc_graph_get_info(mc_ctx *ctx, mc_graph_info *info);
int mc_graph_get_global_masks(mc_ctx *ctx, int32_t *input_index /* M */);
int mc_graph_get_boundary(mc_ctx *ctx, uint8_t *flags /* P */);
int mc_graph_get_point_in_mask(mc_ctx *ctx, uint16_t *pim /* P*F, row-major */);
int mc_graph_get_point_frame_bits(mc_ctx *ctx, uint64_t *bits /* P*ceil(F/64) */);
int mc_graph_get_visible_frame_bits(mc_ctx *ctx, uint64_t *bits /* M*ceil(F/64) */);
int mc_graph_get_contained(mc_ctx *ctx, int64_t *row_off /* M+1 */, int32_t *col_idx /* nnz */);
int mc_graph_get_undersegment(mc_ctx *ctx, int32_t *ids /* |U| */);
int mc_graph_get_nodes0(mc_ctx *ctx, int32_t *mask_index /* N0 */);
int mc_graph_get_observer_hist(mc_ctx *ctx, uint64_t *hist /* F+1 */);
int mc_graph_get_thresholds(mc_ctx *ctx, float *thr /* 20 */, int32_t *is_int /* 20 */, int32_t *n);

/* get_observer_num_thresholds (construction.py:80-96) on an arbitrary
 * visible-frame matrix: rows of ceil(F/64) little-endian uint64 words.       */
int mc_observer_thresholds(mc_ctx *ctx, int32_t num_rows, int32_t num_frames, const uint64_t *vf_bits,
                           float *thr /* 20 */, int32_t *is_int /* 20 */, int32_t *n);

/* ---- S6 on arbitrary nodes (iterative_clustering on user Node lists) ------
 * Replaces the level-0 nodes: per node the visible-frame bits, the contained
 * mask ids (CSR, unique per row) and the point ids (CSR, unique per row).    */
int mc_nodes_set(mc_ctx *ctx, int32_t num_nodes, int32_t num_frames, int32_t num_masks,
                 int64_t num_points, const uint64_t *vf_bits, const int64_t *c_off,
                 const int32_t *c_idx, const int64_t *pt_off, const int32_t *pt_idx);

/* ---- S6: iterative view-consensus clustering ---------------------------
 * thresholds: host array of n values (np.float32 or the int 1), or NULL to
 * use the thresholds computed on the device by mc_graph_build (no host sync).
 * connect_threshold: args.view_consensus_threshold (compared in float32).   */
int mc_cluster_run(mc_ctx *ctx, const float *thresholds, int32_t n, double connect_threshold);
int mc_cluster_get_info(mc_ctx *ctx, mc_cluster_info *info);
/* Edge capture for the set-order replay: with capacity > 0 the next
 * mc_cluster_run records every edge of every iteration as key = t << 48 | a << 24 | b (a < b,
 * any order); mc_cluster_get_edges gives their count (keys NULL) and the keys
 * (MC_ERR_UNSUPPORTED when more than capacity were found).  Single-process runs only. */
int mc_cluster_set_edge_capture(mc_ctx *ctx, int64_t capacity);
int mc_cluster_get_edges(mc_ctx *ctx, uint64_t *keys, int64_t *n);
int mc_cluster_get_level_sizes(mc_ctx *ctx, int32_t *sizes /* num_iterations+1 */);
/* contained-pool slots of every level (sum of the members' row lengths: the merge's row
 * upper bounds), level 0 = nnz of the initial rows; used for the S6 byte models of bench.py */
int mc_cluster_get_level_caps(mc_ctx *ctx, int32_t *caps /* num_iterations+1 */);
int mc_cluster_get_partition(mc_ctx *ctx, int32_t iteration, int32_t *labels /* N_iteration */);
int mc_cluster_get_edge_counts(mc_ctx *ctx, int64_t *edges /* num_iterations */);
int mc_cluster_get_final_labels(mc_ctx *ctx, int32_t *labels /* N0: object of each level-0 node */);
int mc_cluster_get_objects(mc_ctx *ctx, uint64_t *vf_bits /* K*ceil(F/64) */,
                           int64_t *c_off /* K+1 */, int32_t *c_idx,
                           int64_t *pt_off /* K+1 */, int32_t *pt_idx,
                           int64_t *mask_off /* K+1 */, int32_t *mask_idx /* level-0 node ids */);

/* ---- row-block sharding over processes ------------------------------------
 * One process per GPU, each with its own context holding the same scene (mc_scene_set_masks).
 * After mc_shard_set(ctx, rank, world > 1):
 *   - mc_graph_build runs S2 and S3 (graph/construction.py:98-170) on this rank's block of mask
 *     rows only and leaves MC_SHARD_S3 pending;
 *   - mc_shard_import(MC_SHARD_S3) takes every rank's block, runs the under-segmentation undo,
 *     S5 and this rank's tiles of the S4 observer histogram (:80-96), leaves MC_SHARD_HIST pending;
 *   - mc_shard_import(MC_SHARD_HIST) takes the histogram SUMMED over the ranks and computes the
 *     thresholds (the graph is then complete and identical on every rank);
 *   - mc_cluster_run evaluates the first iteration's N0 x N0 pairs (iterative_clustering.py:20-29)
 *     on the rows a = rank (mod world) and leaves MC_SHARD_FOREST pending;
 *   - mc_shard_import(MC_SHARD_FOREST) unites every rank's union-find forest and runs the rest
 *     of S6 (identical on every rank).
 * The host moves the blocks with its own collectives between the calls: mc_shard_export gives
 * this rank's block (size query with dst_dev = NULL; a stream-ordered copy into a device
 * buffer); all-gather the S3 and FOREST blocks into [world][stride_bytes] in rank order; all-reduce
 * (sum, 64-bit) the HIST block.  mc_shard_pending reports the phase waiting (0 = none).
 * world = 1 restores the single-process path. */
#define MC_SHARD_S3 1
#define MC_SHARD_HIST 2
#define MC_SHARD_FOREST 3
int mc_shard_set(mc_ctx *ctx, int32_t rank, int32_t world);
int mc_shard_pending(mc_ctx *ctx, int32_t *phase);
int mc_shard_export(mc_ctx *ctx, int32_t phase, void *dst_dev, int64_t *bytes);
int mc_shard_import(mc_ctx *ctx, int32_t phase, const void *src_dev, int64_t stride_bytes);

/* ---- native collectives ---------------------------------------------------
 * With an RCCL communicator attached, rank and world come from it and the sharded mc_graph_build /
 * mc_cluster_run run their exchanges themselves, stream-ordered on the context stream (S3 rows and
 * union-find forests: ncclAllGather; the observer histogram: ncclAllReduce sum int64; one max
 * all-reduce + host read for the S3 block stride): nothing is left pending for the host.  This is
 * what the Python collectives in maskclustering_amd/graph_shard.py do through torch.distributed.
 * RCCL is loaded (dlopen librccl.so.1) on first use; MC_ERR_UNSUPPORTED if it is absent.
 *   mc_comm_unique_id   ncclGetUniqueId, on one rank; the caller broadcasts the 128 bytes
 *   mc_ctx_comm_init    ncclCommInitRank on the context's device; the context owns the communicator
 *   mc_ctx_attach_comm  a caller-owned ncclComm_t (NULL detaches: back to the single-process path)
 * A communicator of one rank runs the same exchange flow (each collective an identity). */
#define MC_COMM_ID_BYTES 128
int mc_comm_unique_id(uint8_t id[MC_COMM_ID_BYTES]);
int mc_ctx_comm_init(mc_ctx *ctx, const uint8_t id[MC_COMM_ID_BYTES], int32_t rank, int32_t world);
int mc_ctx_attach_comm(mc_ctx *ctx, void *nccl_comm);

/* ---- post-processing of the clustered objects ----------------------
 * Replaces the compute of utils/post_process.py:173-194 (post_process up to export):
 * dbscan_process (:104-123), filter_point (:40-101), merge_overlapping_objects (:7-37).
 * Inputs are host arrays; checks as mc_pp_run_device (the arrays are uploaded and checked by the
 * same kernels: an offset array that is not ascending or exceeds its table, mask_off included, an
 * index out of range and a frame that is not visible are MC_ERR_INVALID, a node spanning more
 * than 2^21 DBSCAN cells is MC_ERR_UNSUPPORTED; of several defects the first in this order is
 * reported).  Nodes are the ones post_process keeps (>= 2 masks, :182), their
 * points in list(node.point_ids) order (graph/node.py:45); node masks are indices into the
 * mask table (mask_point_clouds entries) in node.mask_list order, with the frame column of
 * each.  A node mask whose frame is not among the node's visible frames fails with
 * MC_ERR_INVALID (the reference raises IndexError at :69). */
typedef struct mc_pp_params {
    double dbscan_eps;              /* 0.1   post_process.py:104                    */
    int32_t dbscan_min_points;      /* 4     post_process.py:109                    */
    double point_filter_threshold;  /* args.point_filter_threshold, :95             */
    double overlapping_ratio;       /* 0.8   :194                                   */
} mc_pp_params;

typedef struct mc_pp_info {
    int32_t num_objects;   /* DBSCAN objects of all nodes, node order then class order */
    int32_t num_filtered;  /* objects kept by filter_point                            */
    int32_t num_final;     /* objects left after merge_overlapping_objects            */
    int64_t num_entries;   /* node points in total                                    */
    int64_t num_node_masks;
} mc_pp_info;

int mc_pp_run(mc_ctx *ctx, const mc_pp_params *params, int64_t num_points, int32_t num_frames,
              const double *scene_xyz /* P*3 */, const uint64_t *pfm_bits /* P*ceil(F/64) */,
              int32_t num_masks, const int64_t *mask_off /* num_masks+1 */, const int32_t *mask_pts,
              int32_t num_nodes, const uint64_t *node_vf_bits /* num_nodes*ceil(F/64) */,
              const int64_t *node_pt_off /* num_nodes+1 */, const int32_t *node_pts,
              const int64_t *node_mask_off /* num_nodes+1 */, const int32_t *node_masks,
              const int32_t *node_mask_col);
int mc_pp_get_info(mc_ctx *ctx, mc_pp_info *info);
/* entry_object: object of each node point when the point passes the detection-ratio filter
 * and its object is final, else -1; mask_object / mask_coverage: the object each node mask
 * is assigned to (-1: it intersects none) and its coverage;
 * object_state: 0 dropped by filter_point, 1 merged away, 2 final; object_node; bbox
 * (min xyz, max xyz) per DBSCAN object.  Object ids are DBSCAN object ids. */
int mc_pp_get_results(mc_ctx *ctx, int32_t *entry_object, int32_t *mask_object, double *mask_coverage,
                      uint8_t *object_state, int32_t *object_node, double *object_bbox);

/* mc_pp_run with every array a device pointer (same arguments and layouts).  The checks and the
 * per-node layout run as kernels behind one flag the host reads once: a node mask whose frame is
 * not visible to its node still fails with MC_ERR_INVALID, a node spanning more than 2^21 DBSCAN
 * cells with MC_ERR_UNSUPPORTED.  Inside the call only O(num_nodes + num_objects) words cross
 * between host and device (node offsets and the size order, per-object counts and boxes);
 * nothing proportional to points, mask points or P x F does.  The per-entry results stay on the
 * device; mc_pp_get_info / mc_pp_get_results work as after mc_pp_run (the getter fetches them). */
int mc_pp_run_device(mc_ctx *ctx, const mc_pp_params *params, int64_t num_points, int32_t num_frames,
                     const double *scene_xyz, const uint64_t *pfm_bits, int32_t num_masks, const int64_t *mask_off,
                     const int32_t *mask_pts, int32_t num_nodes, const uint64_t *node_vf_bits,
                     const int64_t *node_pt_off, const int32_t *node_pts, const int64_t *node_mask_off,
                     const int32_t *node_masks, const int32_t *node_mask_col);
/* The same on the context's own S1-S6 result (after mc_cluster_run on a graph built from
 * mc_scene_set_masks), nothing downloaded.  Nodes: the clustered objects with at least 2 level-0
 * masks (post_process.py:182) in object-id order; a node's points: the object's, in the order
 * mc_cluster_get_objects returns them (ascending); its masks: its level-0 members in ascending
 * level-0 node id, each as its row of the mc_scene_set_masks input (which is the mask table of
 * this run) with its frame column; its visible frames: the object's.  This is the canonical-order
 * result: contents follow the reference's algorithm on these orders, not on the reference
 * process's set orders.  scene_xyz: P x 3 float64 on the host or the device,
 * or NULL for the float32 points of mc_scene_set_points widened exactly.  (When the input held
 * masks of frames without points, which the context's table skips, the kept rows' input indices
 * are uploaded: num_masks words.)
 * MC_ERR_STATE: before mc_cluster_run; NULL scene_xyz without points set; nodes given by
 * mc_nodes_set; a sharded context whose exchange is still pending on this rank. */
int mc_pp_run_clustered(mc_ctx *ctx, const mc_pp_params *params, const double *scene_xyz, int scene_on_device);

/* ---- export of the final objects (utils/post_process.py:126-128, 148-165) ---------------------
 * After any of the three mc_pp_run* calls.  Objects are the final ones in DBSCAN-object order
 * (the reference's total_*_list order after the merge).  mc_pp_export_info gives the sizes;
 * mc_pp_export fills the arrays (any pointer may be NULL), host pointers or, with on_device,
 * device pointers:
 *   obj_pt_off [num_final+1], obj_pts     kept points of each object, in its node's point order
 *   obj_mask_off [num_final+1], obj_masks, obj_mask_cov
 *                                         the masks assigned to it, in its node's mask_list order,
 *                                         as mask-table rows, and their coverages
 *   obj_repre [num_final*5]               find_represent_mask: positions into the object's mask
 *                                         list of its five largest coverages (equal coverages in
 *                                         list order, like Python's stable sort), padded with -1
 *   obj_node [num_final]                  the node each object came from
 * mc_pp_export_pred_masks fills the [num_points, num_final] uint8 row-major matrix the
 * reference's prediction npz stores (what mc_eval_match_counts reads). */
int mc_pp_export_info(mc_ctx *ctx, int32_t *num_final, int64_t *num_points, int64_t *num_masks);
int mc_pp_export(mc_ctx *ctx, int64_t *obj_pt_off, int32_t *obj_pts, int64_t *obj_mask_off, int32_t *obj_masks,
                 double *obj_mask_cov, int32_t *obj_repre, int32_t *obj_node, int on_device);
int mc_pp_export_pred_masks(mc_ctx *ctx, uint8_t *out /* num_points*num_final */, int on_device);

/* ---- instance-evaluation match counts -------------------------------
 * Replaces the device part of evaluation/evaluate.py:254-329 (assign_instances_for_scan): per
 * predicted mask k (column k of the [P, K] pred_masks matrix of the prediction npz, non-zero =
 * in the mask, :289): pred_verts[k] = np.count_nonzero (:290), void_intersection[k] (:303) and
 * intersection[k * num_gt + g] = |pred_k ∩ gt instance g| (:308).  gt_instance[p] = index of
 * the ground-truth instance holding point p, or -1. */
int mc_eval_match_counts(mc_ctx *ctx, int64_t num_points, int32_t num_pred, const uint8_t *pred_masks /* P*K */,
                         const int32_t *gt_instance /* P */, int32_t num_gt, const uint8_t *void_flags /* P */,
                         int64_t *pred_verts /* K */, int64_t *void_intersection /* K */,
                         int64_t *intersection /* K*num_gt */);

/* ---- AP evaluation over accumulated scans ------------------------------
 * Replaces evaluation/evaluate.py:254-329 on point lists (no [P, K] prediction matrix, no
 * [K, G] intersection matrix) and :53-205 (evaluate_matches): AP per (class, overlap) over every
 * scan added since mc_ev_begin, equal to the reference's up to the summation order of its final
 * dot product.  The state lives in the context.
 *
 * mc_ev_begin starts or resets an accumulation: the class table (ids in [0, 2e6), distinct), the
 * overlap thresholds as the doubles the caller computed (at most 32), min_region_size, no_class
 * (every ground-truth id becomes id % 1000 + class_ids[0] * 1000 and every prediction has class
 * class_ids[0]).
 *
 * A scan's tables (mc_ev_scan_info / mc_ev_get_scan return the last added scan's):
 *   ground truth  class index, instance id, vert_count: the distinct non-zero ids whose
 *                 id / 1000 is a class id, grouped by class in the table's order, ascending id
 *   predictions   class index, vert_count, void_intersection, score: the kept predictions
 *                 (class in the table, at least min_region_size points) in input order
 *   pairs         (prediction, ground truth, intersection): the non-zero intersections of a
 *                 prediction with the instances of its own class, sorted by (prediction, ground truth)
 *
 * mc_ev_add_scan: gt_ids [num_points] (label * 1000 + k, 0 = none) and the predictions as point
 * lists in CSR form (what mc_pp_export fills; ids within a list distinct), host arrays or, with
 * on_device, device pointers.  pred_classes NULL: class id 0; pred_scores NULL: 1.0.  The range
 * checks (point ids in [0, num_points), gt_ids >= 0, offsets from 0 ascending to num_pred_pts)
 * run in a kernel behind one flag the host reads once; the host does O(instances + predictions
 * + pairs) work.  MC_ERR_INVALID leaves the accumulation as it was.
 * mc_ev_add_scan_clustered: the predictions are the final objects of the context's last
 * mc_pp_run* (class id 0, score 1.0, as export_class_agnostic_mask writes them); MC_ERR_STATE
 * without a post-processing result.
 * mc_ev_add_matches: a scan given as its tables (host arrays).  Ground truths must be grouped by
 * ascending class index; a ground truth's matched predictions are taken in the pair list's order.
 *
 * mc_ev_ap: ap [C * O] (NaN without ground truth, 0 with ground truth but no prediction or no
 * example) and stats [C * O * 4]: examples, true examples, hard false negatives,
 * has_gt | has_pred << 1.  May be called again as scans are added.
 * mc_ev_get_curve: the cell's distinct scores ascending with their (tp, fp, fn); num_scores is
 * always set (0 for a cell without a curve), the arrays may be NULL for the size query. */
int mc_ev_begin(mc_ctx *ctx, int32_t num_classes, const int32_t *class_ids, int32_t num_overlaps, const double *overlaps,
                int64_t min_region_size, int no_class);
int mc_ev_add_scan(mc_ctx *ctx, int64_t num_points, const int32_t *gt_ids /* P */, int32_t num_pred,
                   const int64_t *pred_off /* K+1 */, int64_t num_pred_pts, const int32_t *pred_pts,
                   const int32_t *pred_classes /* K or NULL */, const double *pred_scores /* K or NULL */, int on_device);
int mc_ev_add_scan_clustered(mc_ctx *ctx, const int32_t *gt_ids /* the scene's P */, int on_device);
int mc_ev_add_matches(mc_ctx *ctx, int32_t num_gt, const int32_t *gt_class, const int32_t *gt_id, const int64_t *gt_vert,
                      int32_t num_pred, const int32_t *pred_class, const int64_t *pred_vert, const int64_t *pred_void,
                      const double *pred_score, int64_t num_pairs, const int32_t *pair_pred, const int32_t *pair_gt,
                      const int64_t *pair_int);
int mc_ev_scan_info(mc_ctx *ctx, int32_t *num_gt, int32_t *num_pred, int64_t *num_pairs);
int mc_ev_get_scan(mc_ctx *ctx, int32_t *gt_class, int32_t *gt_id, int64_t *gt_vert, int32_t *pred_class,
                   int64_t *pred_vert, int64_t *pred_void, double *pred_score, int32_t *pair_pred, int32_t *pair_gt,
                   int64_t *pair_int);
int mc_ev_ap(mc_ctx *ctx, double *ap /* C*O */, int64_t *stats /* C*O*4 */);
int mc_ev_get_curve(mc_ctx *ctx, int32_t class_index, int32_t overlap_index, int64_t *num_scores, double *scores,
                    int64_t *tp, int64_t *fp, int64_t *fn);

/* ---- the accumulation as a state buffer: export and merge ---------------------------------------
 * AP depends only on each (class, overlap) cell's multiset of (score, true) examples, its hard
 * false negative count and its has_gt / has_pred flags.  The state buffer holds exactly that, per
 * cell as runs: the distinct scores ascending, each with its count of true and of false examples.
 * It is how per-rank accumulations of a scene-parallel sweep reach one rank (sweep.py) and how a
 * long sweep is checkpointed.
 *
 * The buffer is one contiguous little-endian run of 8-byte-aligned sections (4-byte sections are
 * padded with zeros to a multiple of 8 bytes); cell = class_index * O + overlap_index:
 *   header     int64 [6]       (version << 32) | 0x5645434d ("MCEV"; version 1), C, O,
 *                              min_region_size, no_class (0 / 1), R = runs of all cells
 *   class_ids  int32 [C]       as given to mc_ev_begin
 *   overlaps   double [O]      as given to mc_ev_begin
 *   run_off    int64 [C*O + 1] cell c's runs are run_off[c] .. run_off[c + 1]; from 0 ascending to R
 *   hard_fn    int64 [C*O]
 *   flags      uint32 [C*O]    has_gt | has_pred << 1
 *   key        uint64 [R]      the score as a sortable key: for the double's bits b (-0.0 taken as
 *                              0.0), ~b if b's sign bit is set, else b | 1 << 63; strictly ascending
 *                              within a cell
 *   n_true     uint32 [R]      the run's true examples
 *   n_false    uint32 [R]      its false examples; n_true + n_false >= 1
 * The form is canonical: accumulations with the same multisets, counts and flags export the same
 * bytes, whatever order and grouping their scans arrived in.
 *
 * mc_ev_state_info: the runs, the examples and the buffer's size in bytes (an accumulation without
 * scans: 0 runs).  mc_ev_state_export: the buffer to buf (a device pointer with on_device);
 * MC_ERR_INVALID if bytes is below mc_ev_state_info's.  The runs are computed once and kept until
 * the accumulation changes; neither call changes the accumulation or the last scan's tables.
 *
 * mc_ev_state_merge adds a buffer's examples, hard false negatives (sum) and flags (OR) to the
 * accumulation, as if the buffer's scans had been added to this context; it is no scan
 * (mc_ev_scan_info / mc_ev_get_scan are unchanged).  bytes may exceed the buffer's size (a padded
 * transport buffer); a device buffer must be 8-byte aligned.  The header's sizes are checked against
 * bytes before anything is sized from them; of a device buffer only the header and the per-cell
 * sections come to the host, the runs are checked by a kernel behind one flag word.
 * MC_ERR_INVALID: another configuration than mc_ev_begin's (C, O, class ids in order, overlaps bit
 * for bit, min_region_size, no_class) or a malformed buffer (magic, truncated, offsets not from 0
 * ascending to R, keys not strictly ascending within a cell, a key no score has (NaN), a run
 * without examples, a negative hard_fn, unknown flag bits).  MC_ERR_UNSUPPORTED: the accumulation
 * would reach 2^31 examples.  All checks precede the first write: an error leaves the accumulation
 * as it was. */
int mc_ev_state_info(mc_ctx *ctx, int64_t *num_runs, int64_t *num_examples, int64_t *bytes);
int mc_ev_state_export(mc_ctx *ctx, void *buf, int64_t bytes, int on_device);
int mc_ev_state_merge(mc_ctx *ctx, const void *buf, int64_t bytes, int on_device);

/* ---- frame decode -------------------------------------------------------
 * Replaces the per-frame host work of dataset/scannet.py:49-54 (get_depth: uint16 / depth_scale
 * as float64, stored float32; matterport.py:92 and scannetpp.py:169 alike) and :68-73
 * (get_segmentation(align_with_depth=True): cv2.resize(seg, (W, H), INTER_NEAREST)) for a batch of
 * frames.  Inputs are host arrays, or device pointers when inputs_on_device; outputs are device
 * pointers (e.g. the depth / seg arrays mc_backproject reads).  depth or seg may be NULL. */
int mc_frames_decode(mc_ctx *ctx, int32_t num_frames, int32_t height, int32_t width,
                     const uint16_t *depth /* F*H*W */, double depth_scale, int32_t seg_height, int32_t seg_width,
                     const uint8_t *seg /* F*seg_height*seg_width */, int inputs_on_device,
                     float *depth_out /* device, F*H*W */, uint8_t *seg_out /* device, F*H*W */);

/* ---- open-vocabulary label query ---------------------------------------
 * Replaces the per-object compute of semantics/open-voc_query.py:32-53: for object k, the mean of
 * its representative masks' features (rows obj_rows[obj_off[k] .. obj_off[k+1]) of the
 * num_rows x dim float32 table, summed in that order), its similarity with every label text
 * feature (num_labels x dim), exp(temperature * sim), the softmax and its first argmax (NaN
 * first, like np.argmax; -1 for an object without representative masks).  Float32 like the
 * reference except the dot products, which are summed in float64 and rounded once (the
 * reference's BLAS order is its own). */
int mc_openvoc_query(mc_ctx *ctx, int32_t num_objects, const int64_t *obj_off, const int32_t *obj_rows,
                     int32_t num_rows, int32_t dim, const float *features, int32_t num_labels,
                     const float *label_features, float temperature, int32_t *out_label);

/* ---- CLIP crop preparation for representative masks ----------------------------------------------
 * Replaces the input side of semantics/get_open-voc_features.py:44-99 (CroppedImageDataset.__getitem__
 * with a Resize(bicubic) / ToTensor / Normalize preprocess): per mask (frame index, label) its
 * bounding box in the segmentation frame, `levels` boxes at growing margins (mask2box_multi_level,
 * :49-61), each crop rgb[top:bottom, left:right] pasted into a square of the pad colour (:75-82),
 * resized to out_size x out_size as Pillow's 8-bit bicubic resize does (a square of that size
 * passes through), and written channel-first as ((float32(v) / 255) - mean) / std.  Bit-exact; the
 * model itself is the caller's.  DESIGN.md §2 (f5).
 *
 * Frames: seg uint8 [F, H, W] and rgb uint8 [F, H, W, 3] at one size, host arrays or, with
 * on_device, device pointers (host frames: only the referenced ones are uploaded).  mask_frame /
 * mask_label are host arrays (duplicates allowed, order kept) and are checked before anything is
 * launched: a frame index outside [0, F) or a label outside [0, 255] is MC_ERR_INVALID, as are
 * out_size outside [1, 4096], levels outside [1, 16] and a negative expansion.
 *
 * mc_crop_boxes: boxes [num_masks * levels * 4] = (left, top, right, bottom), right / bottom
 * exclusive as the reference slices, and status [num_masks]: MC_CROP_OK, MC_CROP_ABSENT (no pixel
 * of the label in its frame; the reference's np.min raises; boxes 0) or MC_CROP_EMPTY (a single
 * pixel: every level's crop is 0 x 0).  Outputs are host arrays or, with out_on_device, device
 * pointers; then the call does not wait for the stream.
 * mc_crop_render: one chunk of masks into out, a device pointer to float32 [num_masks, levels, 3,
 * out_size, out_size]; rows of a mask whose status is not MC_CROP_OK are zeros.  boxes / status as
 * mc_crop_boxes wrote them, host arrays (checked: MC_ERR_INVALID for a box outside its frame) or,
 * with boxes_on_device, device pointers (a box outside its frame renders as zeros).  Stream-ordered
 * on the context stream; the call does not wait for it.  Scratch (per crop max(H, W) * out_size * 3
 * bytes and its coefficient table) comes from the context and is bounded by
 * mc_ctx_set_memory_budget (1 GiB when unset): a chunk is rendered in as many launches as that
 * takes, MC_ERR_UNSUPPORTED when one mask alone exceeds it.
 * mc_crop_coeffs: the device-computed table of one (in_size, out_size) in Pillow's layout, for
 * diagnosis and tests: *ksize always; with bounds [out_size * 2] = (first tap, taps) and
 * kk [out_size * ksize] (22-bit fixed point, unused taps 0) both non-NULL, the table. */
#define MC_CROP_OK 0
#define MC_CROP_ABSENT 1
#define MC_CROP_EMPTY 2
typedef struct { int32_t out_size, levels; double expansion; float mean[3], std[3]; uint8_t pad_rgb[3]; } mc_crop_params;
void mc_crop_params_default(mc_crop_params *p);
int mc_crop_boxes(mc_ctx *ctx, int32_t num_frames, int32_t H, int32_t W, const uint8_t *seg, int on_device,
                  int32_t num_masks, const int32_t *mask_frame, const int32_t *mask_label,
                  const mc_crop_params *params, int32_t *boxes, int32_t *status, int out_on_device);
int mc_crop_render(mc_ctx *ctx, int32_t num_frames, int32_t H, int32_t W, const uint8_t *rgb, int on_device,
                   int32_t num_masks, const int32_t *mask_frame, const int32_t *boxes, const int32_t *status,
                   int boxes_on_device, const mc_crop_params *params, float *out);
int mc_crop_coeffs(mc_ctx *ctx, int32_t in_size, int32_t out_size, int32_t *ksize, int32_t *bounds, int32_t *kk);

/* ---- projected boxes of the objects' top views ---------------------------------------------------
 * Replaces get_bbox_by_projection (get_top_images.py:180-237), the reference's only world -> image
 * projection: a request (object, frame) projects the object's points into the frame's camera and
 * takes the pixel bounding box of those that land in the image.  Float64 as the reference:
 * c = world_to_cam * [p, 1] (x, y, z only, each ((r0*x + r1*y) + r2*z) + t without FMA; the
 * reference's BLAS order is its own), points with z > 0 strictly, u = fx * (x / z) + cx and
 * v = fy * (y / z) + cy in three rounded operations each, rounded half to even, in bounds when
 * 0 <= px < width and 0 <= py < height (tested on the rounded float: -0.5 is pixel 0, NaN, +-inf
 * and anything int cannot hold are outside), box = (min px, min py, max px, max py) inclusive.
 * DESIGN.md §2 (f6).  Drawing the box is not part of the library.
 *
 * mc_proj_boxes: points float64 [num_points, 3], or NULL for the mc_scene_set_points points
 * widened exactly (MC_ERR_STATE unless num_points of them are set); the objects' point lists in CSR
 * form (what mc_pp_export fills); intrinsics [num_frames, 4] = fx, fy, cx, cy; world_to_cam
 * [num_frames, 16] row-major (the INVERSE of the reference's camera -> world extrinsics, computed
 * by the caller); requests (req_object[i], req_frame[i]), duplicates allowed, order kept.
 * on_device applies to every input array.  Out: boxes [n * 4], status [n] (MC_PROJ_OK,
 * MC_PROJ_BEHIND: no point with z > 0, the reference returns None at :215-216; MC_PROJ_OUTSIDE: no
 * point in the image, None at :228-229; the box of both is 0) and inside [n] (may be NULL): the
 * number of in-bounds points, 0 without a box.  Host arrays or, with out_on_device, device
 * pointers; then the call does not wait for its kernels (device INPUTS are checked by a kernel whose
 * flag word the host reads first; host inputs are waited for, the uploads read the caller's arrays).  MC_ERR_INVALID, outputs untouched: an object or frame index
 * out of range, offsets not rising from 0, a point id outside [0, num_points), width or height
 * outside [1, 2^30], more than 2^20 requests.
 *
 * mc_proj_top_views: the same on the final objects of the context's last mc_pp_run* (MC_ERR_STATE
 * without one), nothing crossing to the host in between: per final object the first top_k
 * (1 .. 16; the reference draws 9) positions of its mask list by descending coverage, equal
 * coverages in list order (value['mask_list'][:9] after find_represent_mask's in-place sort; the
 * rule of obj_repre), each mask's frame column the request's frame.  points: the scene's float64
 * points (the count mc_pp_run* saw) or NULL as above; num_frames at least the scene's.  Out, each
 * [num_final * top_k] (boxes * 4), -1 where the object has fewer masks: top_pos (positions into the
 * object's mask list of mc_pp_export), top_frame, boxes, status, inside (may be NULL).
 * on_device: points, intrinsics, world_to_cam; out_on_device: the outputs. */
#define MC_PROJ_OK 0
#define MC_PROJ_BEHIND 1
#define MC_PROJ_OUTSIDE 2
int mc_proj_boxes(mc_ctx *ctx, int64_t num_points, const double *points, int32_t num_objects, const int64_t *obj_pt_off,
                  const int32_t *obj_pts, int32_t num_frames, const double *intrinsics, const double *world_to_cam,
                  int32_t width, int32_t height, int32_t num_requests, const int32_t *req_object, const int32_t *req_frame,
                  int on_device, int32_t *boxes, int32_t *status, int32_t *inside, int out_on_device);
int mc_proj_top_views(mc_ctx *ctx, const double *points, int32_t num_frames, const double *intrinsics,
                      const double *world_to_cam, int32_t width, int32_t height, int on_device, int32_t top_k,
                      int32_t *top_pos, int32_t *top_frame, int32_t *boxes, int32_t *status, int32_t *inside,
                      int out_on_device);

/* ---- scene point cloud from RGB-D frames ------------------------------------------------------------
 * Replaces backproject + create_downsampled_point_cloud (tasmap/tasmap2mct_format.py:216-284), the
 * producer of a TASMap scene's points.  DESIGN.md §2 (f7).
 *
 * mc_cloud_fuse_frames: frames in order; depth float32 [F, H, W] (metres), rgb uint8 [F, H, W, 3],
 * intrinsics float64 [F, 4] = fx, fy, cx, cy, poses float64 [F, 16] row-major camera -> world;
 * on_device applies to all four.  A pixel (v, u) is kept iff 0 < d < depth_trunc (NaN, +-inf, 0,
 * negative and d == depth_trunc are dropped), pixels row-major; its point is S1's (z = (double)d,
 * x = ((u - cx) z) / fx, y = ((v - cy) z) / fy, the pose as ((T0 x + T1 y) + T2 z) + T3 per row without
 * FMA, then the divide by row 3); its colour (r, g, b) / 255.0 in float64.  buffer_frames consecutive
 * frames make a buffer, flushed when (i + 1) % buffer_frames == 0 and, if non-empty, after the
 * last frame; a flush is voxel_down_sample(voxel_size) of the buffer's points, frame-major then
 * pixel order; the flushed results are concatenated in order and voxel_down_sample'd once more.
 * voxel_down_sample: vmin = min - voxel / 2 per axis, index = floor((p - vmin) / voxel) (a rounded
 * subtraction, a rounded division), a voxel's sums of points and colours are the LEFT FOLD IN INPUT
 * ORDER in float64, mean = sum / count, output order = order of each voxel's first input point.
 * (Open3D's own order and summation order are its hash map's: parity-unpinned, as for S1.)
 * The result stays on the device with the context.  An empty result (no valid pixel, F == 0) is valid.
 *
 * mc_cloud_voxel_down: one voxel_down_sample of points float64 [n, 3] with colours float64 [n, 3] or
 * NULL (then the result has no colours), by the same device routine.
 *
 * mc_cloud_info: out[5] = result points, voxel_down_sample runs of the call (empty ones included),
 * the largest run's input points, the largest voxel population seen, bytes the result holds.
 * mc_cloud_get: the result's points and colours (float64 [n, 3] each; either may be NULL) to host
 * arrays or, with on_device, device pointers.
 * mc_scene_use_cloud: the result's points rounded to float32 (to nearest) become the scene points,
 * on the device; equal in effect to mc_scene_set_points of that array.
 *
 * Every check precedes the first write of context state: a refused call leaves the earlier result.
 * MC_ERR_INVALID: a non-finite pose or intrinsic entry, voxel_size <= 0, buffer_frames < 1, a
 * non-finite point.  MC_ERR_UNSUPPORTED: a voxel_down_sample run spanning 2^21 voxels or more on an
 * axis, one of 2^31 points or more, one whose arrays exceed mc_ctx_set_memory_budget (the message
 * names the bytes; without a budget four fifths of the free device memory).  MC_ERR_STATE:
 * mc_cloud_info, mc_cloud_get or mc_scene_use_cloud before a result, colours of a result without. */
typedef struct { double voxel_size, depth_trunc; int32_t buffer_frames; } mc_cloud_params;
void mc_cloud_params_default(mc_cloud_params *p);
int mc_cloud_fuse_frames(mc_ctx *ctx, int32_t num_frames, int32_t height, int32_t width, const float *depth,
                         const uint8_t *rgb, const double *intrinsics, const double *poses, int on_device,
                         const mc_cloud_params *params);
int mc_cloud_voxel_down(mc_ctx *ctx, int64_t num_points, const double *points, const double *colors, double voxel_size,
                        int on_device);
int mc_cloud_info(mc_ctx *ctx, int64_t *out5);
int mc_cloud_get(mc_ctx *ctx, double *points, double *colors, int on_device);
int mc_scene_use_cloud(mc_ctx *ctx);

/* ---- label images from per-frame instance masks -------------------------------------------------------
 * Replaces the end of step 1 (mask_predict.py:94-113): a 2-D model's instance masks become the uint8
 * label image S1 reads, ids 1..K by ascending score, at most 255 per frame.  DESIGN.md §2 (f8).
 *
 * mc_labels_paint: frames are ragged; frame f owns instances inst_off[f] .. inst_off[f+1]) (host array,
 * F + 1 entries from 0, non-decreasing; an empty frame yields zeros).  masks [inst_off[F], H, W] of
 * mask_dtype (MC_PAINT_U8: uint8 or bool bytes, MC_PAINT_F32: float32), scores float32 [inst_off[F]];
 * on_device applies to both.  Per frame:
 *   1. instance i is selected iff score[i] >= score_threshold, compared in float32 (a NaN score never is);
 *   2. selected instances are ordered by ascending score, EQUAL SCORES (-0.0 and +0.0 included) BY
 *      ASCENDING INSTANCE INDEX (torch's CPU sort gives this order; its CUDA sort does not promise one:
 *      parity-unpinned on ties);
 *   3. in that order an instance whose area is < min_pixels is skipped and takes no id; every other one
 *      is kept, takes the next id from 1 and sets every pixel of its mask to it, later ones overwriting
 *      earlier ones.  The area is the whole mask's: a kept instance may own no pixel and still takes its id;
 *   4. a pixel is set iff its value EQUALS 1 (uint8 1, float32 1.0); the area is the number of set
 *      pixels, which is the reference's torch.sum for 0/1 masks (for other values it differs: a
 *      documented deviation);
 *   5. a frame with more than 255 kept instances (numpy raises OverflowError at the 256th) gets status
 *      MC_PAINT_OVERFLOW, an all-zero image and a label_instance row of -1; the other frames are painted.
 * labels_out is always a device pointer, uint8 [F, H, W] (it can go to mc_frames_decode with
 * inputs_on_device or to mc_backproject with on_device).  The four small outputs may each be NULL and
 * are host arrays or, with out_on_device, device pointers: status [F], num_kept [F] (the kept count,
 * above 255 on overflow), label_instance [F * 255] (the index within its frame of the instance with id
 * k + 1; -1 beyond num_kept), instance_area [inst_off[F]] (set pixels of every instance, selected or not).
 * A call with host inputs or host outputs waits for the stream; one with device inputs and device
 * outputs does not.
 *
 * Scratch (one bit per mask value and, for host inputs, the staged masks) comes from the context and
 * respects mc_ctx_set_memory_budget (1 GiB when unset): the frames are painted in rounds that fit;
 * MC_ERR_UNSUPPORTED when one frame alone does not.  Every refusal precedes the first launch and the
 * first write of context state.  MC_ERR_INVALID: inst_off not non-decreasing from 0, a frame with more
 * than MC_PAINT_MAX_INSTANCES instances, an unknown mask_dtype, non-positive H or W, H * W > 2^31 - 1,
 * a negative min_pixels or num_frames, a missing array. */
typedef struct { float score_threshold; int32_t min_pixels; } mc_paint_params;   /* 0.5f, 400 */
#define MC_PAINT_OK 0
#define MC_PAINT_OVERFLOW 1
#define MC_PAINT_MAX_INSTANCES 1024  /* per frame */
#define MC_PAINT_U8 0
#define MC_PAINT_F32 1
void mc_paint_params_default(mc_paint_params *p);
int mc_labels_paint(mc_ctx *ctx, int32_t num_frames, int32_t H, int32_t W, const int64_t *inst_off, int32_t mask_dtype,
                    const void *masks, const float *scores, int on_device, const mc_paint_params *params,
                    uint8_t *labels_out, int32_t *status, int32_t *num_kept, int32_t *label_instance,
                    int32_t *instance_area, int out_on_device);

/* host utility: packed little-endian bit rows (bit c of word c/64 = column c) -> one byte per
 * column, rows * ncols bytes (the dense bool point_frame_matrix the reference's callers read,
 * graph/construction.py:40,52), split over host threads.                                      */
int mc_bits_unpack(const uint64_t *words, int64_t rows, int32_t words_per_row, int32_t ncols, uint8_t *out);

/* host utility: the reference's container ORDERS of the clustering result (graph/iterative_clustering.py:5-10
 * + graph/node.py:24-37 under networkx 3.x's _plain_bfs and CPython's set tables; mc_setorder.inl).
 * Iterations t = 0 .. num_levels-1 with level_sizes[t] nodes; iteration t's edges (a, b), a != b, are
 * edge_a/edge_b[edge_off[t] .. edge_off[t+1]) (level_sizes[t+1] must be the number of components of t).
 * Level-0 node i's point set was made by adding pts[pt_off[i] .. pt_off[i+1]) in order to an empty set.
 * Out (caller-allocated, K = *num_objects = components of the last iteration <= level_sizes[T-1]):
 *   obj_mask_off [K+1] + mask_order [level_sizes[0]]: final node k's mask_list as level-0 node indices;
 *   obj_pt_off [K+1] + obj_pts [<= pt_off[level_sizes[0]]]: list(final node k's point_ids);
 *   son_off [K+1] + son_order [level_sizes[T-1]]: the last iteration's members of k in set order;
 *   labels [sum_t level_sizes[t]] (NULL: not returned): component of every node of every iteration.
 * num_threads <= 0: all host threads.                                                                 */
int mc_setorder_replay(int32_t num_levels, const int32_t *level_sizes, const int64_t *edge_off,
                       const int32_t *edge_a, const int32_t *edge_b, const int64_t *pt_off, const int32_t *pts,
                       int32_t num_threads, int32_t *num_objects, int64_t *obj_mask_off, int32_t *mask_order,
                       int64_t *obj_pt_off, int32_t *obj_pts, int64_t *son_off, int32_t *son_order,
                       int32_t *labels);

/* The same in two calls, so that the level-0 sets are built while the device clusters: begin takes
 * level-0 node i's points as pts[node_start[i] .. node_start[i] + node_len[i]) (rows of the caller's
 * mask CSR, no flattened copy) and, with async_build != 0, builds the sets on a background thread
 * (the caller keeps node_start / node_len / pts alive until finish or free); finish waits for it and
 * replays the iterations exactly as mc_setorder_replay (outputs as there; obj_pts holds at most
 * sum(node_len)).  finish is called at most once; free joins and releases (also after an error). */
typedef struct mc_setorder mc_setorder;
int mc_setorder_begin(int32_t num_nodes, const int64_t *node_start, const int64_t *node_len, const int32_t *pts,
                      int32_t num_threads, int async_build, mc_setorder **out);
int mc_setorder_finish(mc_setorder *h, int32_t num_levels, const int32_t *level_sizes, const int64_t *edge_off,
                       const int32_t *edge_a, const int32_t *edge_b, int32_t *num_objects, int64_t *obj_mask_off,
                       int32_t *mask_order, int64_t *obj_pt_off, int32_t *obj_pts, int64_t *son_off,
                       int32_t *son_order, int32_t *labels);
void mc_setorder_free(mc_setorder *h);

#ifdef __cplusplus
}
#endif
#endif /* MCGRAPH_H */
