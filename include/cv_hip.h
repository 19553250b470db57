/*
 * cv_hip.h -- C ABI of libcvhip.so, the MI355X (gfx950) implementation of the
 * CanonicalVoting hot path.  Plain pointers and sizes only: every `d_` pointer is
 * device memory owned by the caller, every `h_` pointer is host memory, `stream`
 * is a hipStream_t passed as void* (NULL = the legacy default stream).
 *
 * All entry points return 0 on success or a negative CV_E* code; nothing throws
 * across this boundary.  cv_last_error() returns a thread-local message for the
 * last failing call.
 *
 * Each group cites the reference interface it replaces (paths relative to the
 * reference checkout).  The Python binding that presents these under the
 * reference's names (`hv_cuda.forward/backward`, `HoughVoting`, `MinkowskiEngine`
 * facade, `MinkUNet34C`) lives in canonicalvoting_amd/; INTEGRATION.md shows the
 * stub a reference maintainer would add.
 */
#ifndef CV_HIP_H
#define CV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CV_OK 0
#define CV_EINVAL (-22)   /* bad argument (null pointer, negative size, unsupported value) */
#define CV_ENOMEM (-12)   /* workspace too small */
#define CV_EHIP (-5)      /* a HIP runtime call or kernel launch failed */
#define CV_ERANGE (-34)   /* result does not fit the caller's buffers */

/* Version of this header.  cv_abi_version() returns the value the LIBRARY was built with: a binding compiled against
 * this header compares the two (csrc/hv_cuda_ext.cpp does at import) and refuses a stale pair.
 * 2 (round 5): neighbour windows (cv_sp_build_windows, cv_conv_desc.win, cv_scene_maps.win, win_levels arguments of the
 *    scene-plan calls, `wins` of cv_net_run_f32); the round 1-3 tile-plan symbols are gone.
 * 3 (round 6): launch sizing per call - cv_scene_desc.conv_split_target / vote_part_records, cv_hv_set_part_records_thread;
 *    cv_sp_copy_unless_flag, cv_sp_pack_weights_h2_batch_f32; the neighbour windows of round 5 (conv_win: exact, measured slower
 *    than the mask-sorted kernels at every level, LABNOTES round 5) are gone - cv_sp_build_windows, cv_conv_desc.win,
 *    cv_scene_maps.win, the win_levels arguments and cv_net_win_levels.
 * 4: cv_sp_scene_plan_layout, cv_sp_scene_plan_slots, cv_sp_scene_conv_workspace_bytes (additive: no struct or signature moved).
 * 5: the model axis - cv_net_run_models_f32 with its size / table helpers, cv_head_separate_models_f32,
 *    cv_scene_separate_desc.models_per_pass / d_model_params (appended: a zero-initialised descriptor runs as before).
 * 6: raw clouds - cv_sp_voxel_rows_f32 (cv_gather_job), cv_detect_points_f32, cv_detect_points_separate_f32 with their
 *    descriptors / results and the cv_sizeof_* helpers (additive: no struct or signature moved).
 *    Since then, still 6: cv_hv_forward_peaks_f32 / cv_hv_forward_peaks_cat_f32 and a trailing cv_scene_desc.peak_quotients
 *    (appended: a zero-initialised descriptor runs as before; cv_scene_separate_desc has no such field, its scene call votes full
 *    grids).
 *    Still 6: cv_sp_scan_rows_f32 (cv_scan_rows_desc) and cv_sizeof_scan_rows_desc, the training batch from raw scans
 *    (additive: no struct or signature moved).
 *    Still 6: cv_sym_loss_fwd_f32 / cv_sym_loss_bwd_f32 (cv_sym_loss_desc) with cv_sym_loss_workspace_bytes,
 *    cv_sym_loss_chunk_rows and cv_sizeof_sym_loss_desc, the separate-model coordinate loss over packed symmetry labels
 *    (additive: no struct or signature moved).
 *    Still 6: cv_sp_sym_rows_f32 (cv_sym_rows_desc) with cv_sp_sym_rows_workspace_bytes, cv_sp_sym_rows_block,
 *    cv_sp_sym_rows_scan_span and cv_sizeof_sym_rows_desc, the separate-model training batch (packed symmetry labels and row
 *    arrays) from raw scans (additive: no struct or signature moved).
 *    Still 6: cv_row_loss_fwd_f32 / cv_row_loss_bwd_f32 (cv_row_loss_desc) with cv_row_loss_workspace_bytes,
 *    cv_row_loss_chunk_rows and cv_sizeof_row_loss_desc, the per-row training losses of both models (masked squared errors of
 *    the chosen head and the cross entropy) and the validation form of the joint one (additive: no struct or signature moved).
 *    Still 6: a trailing cv_conv_desc.valid_words (appended: a zero-initialised descriptor runs as before).
 *    Still 6: the scene axis - cv_decode_scenes_f32 (cv_decode_scene_job) with cv_decode_scenes_workspace_bytes,
 *    cv_detect_scenes_f32 (cv_scenes_desc, cv_scenes_result) and their cv_sizeof_* helpers (additive: no struct or signature
 *    moved).
 *    Still 6: the vote's scene axis - cv_hv_forward_scenes_f32 / cv_hv_forward_peaks_scenes_f32 over cv_decode_scene_job with
 *    cv_hv_forward_scenes_workspace_bytes (additive: no struct or signature moved). */
#define CV_ABI_VERSION 6
int cv_abi_version(void);
const char* cv_last_error(void);

/* ------------------------------------------------------------------------ *
 * Vote op: replaces pybind module `hv_cuda`
 *   forward  <- houghvoting/src/hv_cuda.cpp:30-45  -> hv_cuda_kernel.cu:121-165
 *   backward <- houghvoting/src/hv_cuda.cpp:47-71  -> hv_cuda_kernel.cu:265-302
 * ------------------------------------------------------------------------ */

/* Axis-aligned bounds of d_points[n][3] (torch::min/max(points,0),
 * hv_cuda_kernel.cu:129).  Writes h_min3/h_max3 and synchronises `stream` once.
 * d_ws: >= cv_hv_minmax_workspace_bytes() bytes of device scratch. */
size_t cv_hv_minmax_workspace_bytes(void);
int cv_hv_minmax_f32(const float* d_points, int64_t n, float* h_min3, float* h_max3,
                     void* d_ws, size_t ws_bytes, void* stream);
/* The same reduction without the host wait: h_minmax6 must be PINNED host memory (min xyz, max xyz) and is
 * valid once the work enqueued on `stream` up to this call has completed.  A pipeline can start it before the
 * network forward of a scene, so the vote does not stall on the grid shape (hv_cuda_kernel.cu:129-134 blocks
 * the host twelve times at that point). */
int cv_hv_minmax_async_f32(const float* d_points, int64_t n, float* h_minmax6, void* d_ws, size_t ws_bytes,
                           void* stream);

/* Grid shape from the bounds in the reference's fp32 arithmetic
 * (hv_cuda_kernel.cu:131-134: trunc((max-min)/res) + 1).  Host only. */
int cv_hv_grid_dims_f32(const float h_min3[3], const float h_max3[3], float res, int dims_out[3]);

/* algo: 0 = auto, 1 = direct global fp32 atomics (+memset +normalise pass),
 *       2 = LDS-tiled accumulation with fused normalise (no global atomics).
 * Any other value is refused: the forward calls and the scene descriptors (vote_algo) return CV_EINVAL before they touch
 * the GPU, the two workspace queries return 0. */
size_t cv_hv_forward_workspace_bytes(int64_t n, int num_rots, const int dims[3], int algo);

/* Vote accumulation + per-cell normalisation (hv_cuda_kernel.cu:12-119).
 * d_grid_obj[X][Y][Z], d_grid_rot[X][Y][Z][2], d_grid_scale[X][Y][Z][3] are fully
 * overwritten (no pre-zeroing needed).  h_corner3 = grid origin (min of points, or
 * corners[0] for the 7-argument SUN RGB-D variant, sunrgbd/brnetcanon.py:99).
 * Asynchronous on `stream`. */
int cv_hv_forward_f32(const float* d_points, const float* d_xyz, const float* d_scale,
                      const float* d_obj, int64_t n, float res, int num_rots,
                      const float h_corner3[3], const int dims[3], float* d_grid_obj,
                      float* d_grid_rot, float* d_grid_scale, void* d_ws, size_t ws_bytes,
                      int algo, void* stream);

/* Category axis (separate mode, eval_separate.py:166-186: one grid triple per category over the SAME scan points, corner and
 * grid shape).  K = num_cats categories, 1 <= K <= CV_MAX_CATEGORIES, in one launch sequence whose launch count does not depend
 * on K: d_xyz / d_scale [K][n][3], d_obj [K][n] in; d_grid_obj [K][X][Y][Z], d_grid_rot [K][X][Y][Z][2],
 * d_grid_scale [K][X][Y][Z][3] out.  Category k is bit for bit what cv_hv_forward_f32 writes for that category alone
 * (cv_hv_forward_f32 is the K = 1 case of the same launches).  The workspace is K carves of the single-category size
 * (cv_hv_forward_cat_workspace_bytes(.., 1) == cv_hv_forward_workspace_bytes).  Asynchronous on `stream`. */
#define CV_MAX_CATEGORIES 16
size_t cv_hv_forward_cat_workspace_bytes(int64_t n, int num_rots, const int dims[3], int algo, int num_cats);
int cv_hv_forward_cat_f32(const float* d_points, const float* d_xyz, const float* d_scale, const float* d_obj, int64_t n,
                          float res, int num_rots, const float h_corner3[3], const int dims[3], int num_cats, float* d_grid_obj,
                          float* d_grid_rot, float* d_grid_scale, void* d_ws, size_t ws_bytes, int algo, void* stream);

/* The vote for a caller that only decodes.  The decode reads d_grid_rot / d_grid_scale in one place, the compaction of the
 * cells with d_grid_obj >= thresh_high, so these variants accumulate the five quotient numerators only there: one launch of the
 * tile kernel for the objectness channel alone (it also notes, per plane and tile, the box of its cells >= thresh), a second one
 * over the tiles that hold such a cell.  Arguments as cv_hv_forward_f32 / cv_hv_forward_cat_f32 plus `thresh` (not NaN;
 * -INFINITY makes every cell count).  d_grid_obj is written everywhere and is bit for bit what the full call writes;
 * d_grid_rot / d_grid_scale HOLD VALUES ONLY WHERE d_grid_obj >= thresh - there the same bits as the full call's (every sum is
 * an integer) - and are left untouched elsewhere.  The same workspace as the full call:
 * cv_hv_forward_workspace_bytes covers the boxes (16 bytes per plane and tile) and the list of work items the second launch walks
 * (16 bytes per workgroup of the full launch) for every caller, 0.2 MB at 80k points.  algo 1 (direct) has no such variant:
 * it writes full grids.  Asynchronous on `stream`; no host wait, the boxes stay on the device. */
int cv_hv_forward_peaks_f32(const float* d_points, const float* d_xyz, const float* d_scale, const float* d_obj, int64_t n,
                            float res, int num_rots, const float h_corner3[3], const int dims[3], float* d_grid_obj,
                            float* d_grid_rot, float* d_grid_scale, void* d_ws, size_t ws_bytes, int algo, float thresh,
                            void* stream);
int cv_hv_forward_peaks_cat_f32(const float* d_points, const float* d_xyz, const float* d_scale, const float* d_obj, int64_t n,
                                float res, int num_rots, const float h_corner3[3], const int dims[3], int num_cats,
                                float* d_grid_obj, float* d_grid_rot, float* d_grid_scale, void* d_ws, size_t ws_bytes, int algo,
                                float thresh, void* stream);

/* Launch sizing of the vote's streaming launch: records of a plane's two y-bins that one workgroup of a (tile, plane) takes; a
 * plane with more is split over up to 8 workgroups per tile whose partial tiles the last arriver adds (integer sums: the grids
 * are the same bits under every setting).  Default 4096 (or CV_HV_PART_RECORDS) - the fastest kernel for ONE scene in flight;
 * a host that keeps several scenes in flight sets a larger value (bench.py: 12288 from four scenes in flight: fewer, longer
 * workgroups and less merge traffic while the other scenes fill the chip; 574 -> 585 scenes/s with seven).  Values below 4096 are raised to it (the workspace
 * bound assumes it); records <= 0 restores the default.  Returns the previous value.  Process-wide, like
 * cv_sp_set_split_target. */
int cv_hv_set_part_records(int records);
/* The same for the CALLING THREAD's launches only (0 = follow the process-wide value); returns the previous thread value.
 * cv_detect_scene_f32 sets it from cv_scene_desc.vote_part_records for the duration of the call. */
int cv_hv_set_part_records_thread(int records);
/* Measurement hook (no reference counterpart): the CALLING THREAD's following cv_hv_forward_f32 calls record the two
 * hipEvent_t handles directly before and after the accumulation kernel of the tile algorithm (hv_fwd_tiles; the peaks
 * variants: before the first and after the second of their two launches - the whole accumulation), on the
 * stream of the call - bench.py times exactly the kernel its `roofline` prices, with other scenes in flight, instead
 * of the whole op.  NULL, NULL switches it off.  The events stay the caller's. */
int cv_hv_set_kernel_events(void* ev_start, void* ev_stop);

/* Gradient of sum(grad_obj * grid_obj) wrt xyz/scale/obj (hv_cuda_kernel.cu:168-261),
 * including the reference's missing 1/res factor.  Outputs are overwritten.
 * Asynchronous on `stream`. */
int cv_hv_backward_f32(const float* d_grad_obj, const float* d_points, const float* d_xyz,
                       const float* d_scale, const float* d_obj, int64_t n, float res,
                       int num_rots, const float h_corner3[3], const int dims[3], float* d_dxyz,
                       float* d_dscale, float* d_dobj, void* stream);

/* Number of (point, rotation) votes that pass the bounds test
 * (hv_cuda_kernel.cu:41-44); used for the algorithmic byte count of DESIGN.md.
 * Synchronises `stream`. */
int cv_hv_count_votes_f32(const float* d_points, const float* d_xyz, const float* d_scale, int64_t n,
                          float res, int num_rots, const float h_corner3[3], const int dims[3],
                          int64_t* h_count, void* d_ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * Detection decode: replaces the inline loop eval_joint.py:195-263
 * (duplicated at train_joint.py:355-439, train_separate.py:371-431,
 * eval_separate.py:195-264) and the per-class NMS eval_joint.py:75-89,270-280
 * with utils/calc_map.py:6-21 as the IoU.
 * ------------------------------------------------------------------------ */
typedef struct cv_decode_params {
    float thresh_high;  /* eval_joint.py:18  (60)  */
    float thresh_low;   /* eval_joint.py:19  (10)  */
    float valid_ratio;  /* eval_joint.py:20  (0.2) */
    int elimination;    /* eval_joint.py:21  (2)   */
    float prob_thresh;  /* eval_joint.py:245 (0.3) */
    int elim_hi_plus1;  /* 1 = eval_joint.py:211 slice, 0 = eval_separate.py:209 slice */
    int max_iters;      /* capacity of the h_* output arrays (candidates examined) */
    double err_thresh;  /* eval_joint.py:252 (0.3) */
} cv_decode_params;

size_t cv_decode_workspace_bytes(const int dims[3], int64_t n, int max_iters);

/* Greedy peak picking + grid suppression + back-projection check + class vote.
 * Device inputs are read-only unless mutate_grid != 0, in which case d_grid_obj
 * receives the same zeroing the reference applies in place (:211,:243).
 * Host outputs: h_n_cand candidates examined (cell index + verdict 0 accept /
 * 1 too few confident points / 2 LCC error), h_n_boxes accepted boxes in
 * acceptance order (corners [8][3], score, class).  *h_truncated (may be NULL) is set to 1 when max_iters candidates
 * were examined and a cell >= thresh_high is still live - the reference's `while True` loop (:204-209) would have gone
 * on, so the caller must re-run with a larger max_iters rather than use the result.  Synchronises `stream` once. */
int cv_decode_f32(float* d_grid_obj, const float* d_grid_rot, const float* d_grid_scale,
                  const int dims[3], const float h_corner3[3], float res, const float* d_points,
                  const float* d_xyz, const float* d_prob, const int32_t* d_class, int64_t n,
                  const cv_decode_params* params, int mutate_grid, void* d_ws, size_t ws_bytes,
                  int* h_n_cand, int64_t* h_cand_idx, int32_t* h_verdict, int* h_n_boxes,
                  float* h_boxes, float* h_scores, int32_t* h_classes, int* h_truncated, void* stream);

/* cv_decode_f32 over K = num_cats categories with ONE host wait (separate mode: each category's grid triple is decoded on
 * its own, eval_separate.py:195-264).  Grids [K][X][Y][Z] (+[2], [3]) as cv_hv_forward_cat_f32 writes them, d_xyz [K][n][3],
 * d_prob [K][n]; d_points [n][3] and d_class [n] are shared (d_class NULL: class 0 for every point, as separate mode passes
 * it).  Per category k the host outputs land at h_n_cand[k], h_n_boxes[k], h_truncated[k] (may be NULL) and the arrays at
 * k * max_iters entries (h_boxes: k * max_iters * 24 floats): category k is exactly what cv_decode_f32 returns for it
 * alone.  The greedy walks of the K categories run side by side (one walker workgroup each).  Synchronises once. */
size_t cv_decode_cat_workspace_bytes(const int dims[3], int64_t n, int max_iters, int num_cats);
int cv_decode_cat_f32(float* d_grid_obj, const float* d_grid_rot, const float* d_grid_scale, const int dims[3],
                      const float h_corner3[3], float res, const float* d_points, const float* d_xyz, const float* d_prob,
                      const int32_t* d_class, int64_t n, int num_cats, const cv_decode_params* params, int mutate_grid, void* d_ws,
                      size_t ws_bytes, int* h_n_cand, int64_t* h_cand_idx, int32_t* h_verdict, int* h_n_boxes, float* h_boxes,
                      float* h_scores, int32_t* h_classes, int* h_truncated, void* stream);

/* cv_decode_f32 over B = num_scenes scenes with ONE host wait.  Unlike the categories above, scenes share nothing but the
 * parameters: job b has its own grid shape, corner and grid triple, and its points are the rows [row0, row0 + n) of the shared
 * d_points / d_xyz [.][3], d_prob / d_class [.] arrays (d_class is required).  1 <= B <= CV_MAX_SCENES.  d_ws:
 * cv_decode_scenes_workspace_bytes(jobs, B, max_iters) bytes - the sum of the jobs' cv_decode_workspace_bytes, carved in job
 * order.  Scene b's host outputs land at h_n_cand[b], h_n_boxes[b], h_truncated[b] (may be NULL) and the arrays at
 * b * max_iters entries (h_boxes: b * max_iters * 24 floats): exactly what cv_decode_f32 returns for that scene alone,
 * mutate_grid included.  The B greedy walks run side by side, each on the walker workgroup the single call would choose for
 * its grid.  CV_EINVAL (the message names the scene) before anything is launched.  Synchronises once. */
#define CV_MAX_SCENES 16
typedef struct cv_decode_scene_job {
    float* d_grid_obj; const float* d_grid_rot; const float* d_grid_scale;      /* [X][Y][Z] (+[2], [3]) */
    int dims[3];
    float corner[3];
    int64_t row0, n;              /* the scene's rows of the shared arrays */
} cv_decode_scene_job;
size_t cv_decode_scenes_workspace_bytes(const cv_decode_scene_job* jobs, int num_scenes, int max_iters);
int cv_decode_scenes_f32(const cv_decode_scene_job* jobs, int num_scenes, float res, const float* d_points, const float* d_xyz,
                         const float* d_prob, const int32_t* d_class, const cv_decode_params* params, int mutate_grid, void* d_ws,
                         size_t ws_bytes, int* h_n_cand, int64_t* h_cand_idx, int32_t* h_verdict, int* h_n_boxes, float* h_boxes,
                         float* h_scores, int32_t* h_classes, int* h_truncated, void* stream);

/* cv_hv_forward_f32 / cv_hv_forward_peaks_f32 over B = num_scenes scenes in ONE launch sequence whose launch count does not
 * depend on B, on the job table the decode above takes: a caller builds one table and hands it to the vote and then to the
 * decode.  The vote WRITES through d_grid_rot / d_grid_scale (declared const for the decode, which reads them).  Job b votes the
 * rows [row0, row0 + n) of the shared d_points / d_xyz / d_scale [.][3] and d_obj [.] arrays onto its own corner and shape into
 * its own grid triple; row ranges may come in any order and leave gaps, nothing outside a job's range is read.  Every job's
 * grids are bit for bit what the single call writes for that scene alone, on every launch shape (all sums are integers).
 * 1 <= B <= CV_MAX_SCENES; B = 1 is the single call.  d_ws: cv_hv_forward_scenes_workspace_bytes(jobs, B, num_rots, algo)
 * bytes - the sum of the jobs' cv_hv_forward_workspace_bytes, carved in job order; it may arrive dirty.  When algo resolves to
 * the direct kernel (more than 256 rotations) the jobs run one after another.  cv_hv_set_kernel_events (around the accumulation
 * launches) and cv_hv_set_part_records[_thread] (one part size for all jobs) apply as to the single call.  CV_EINVAL (the
 * message names the scene) before anything is launched.  Asynchronous on `stream`: no host wait, no allocation. */
size_t cv_hv_forward_scenes_workspace_bytes(const cv_decode_scene_job* jobs, int num_scenes, int num_rots, int algo);
int cv_hv_forward_scenes_f32(const cv_decode_scene_job* jobs, int num_scenes, const float* d_points, const float* d_xyz,
                             const float* d_scale, const float* d_obj, float res, int num_rots, void* d_ws, size_t ws_bytes,
                             int algo, void* stream);
int cv_hv_forward_peaks_scenes_f32(const cv_decode_scene_job* jobs, int num_scenes, const float* d_points, const float* d_xyz,
                                   const float* d_scale, const float* d_obj, float res, int num_rots, void* d_ws, size_t ws_bytes,
                                   int algo, float thresh, void* stream);

/* Instance labels: which scan points each of a list of boxes owns (eval_joint.py:231-245: bbox_mask_world and mask, which
 * the decode reduces to statistics per candidate and drops).  A box is named by the flat grid cell the decode examined
 * as a candidate; its geometry is formed from the grids exactly as the decode formed it (rotation by double-rounded
 * atan2 / cos / sin of the rot cell, scale from the scale cell, centre h_corner3[d] + res * cell_d in fp32), so membership
 * agrees with the decode's in-box test on every point, the ones on a face included.  A point is a member of a box when
 * it lies strictly inside it and - with confident_only - d_prob[i] > prob_thresh (strict: a NaN prob is not confident).
 * Its owner is the FIRST box of the category's list that has it as a member: the list order is the priority.
 * Grids [K][X][Y][Z][2|3], d_points [n][3] shared by the categories, d_prob [K][n] (may be NULL when confident_only == 0),
 * h_cells / h_label_of [K][max_boxes] host arrays of which the first h_n_boxes[k] entries of row k are read (they may be
 * reused as soon as the call returns).  d_owner [K][n] receives h_label_of of the owning box, -1 where no box has the
 * point (h_n_boxes[k] == 0: -1 everywhere).  d_count_in / d_count_owned [K][max_boxes] (each may be NULL): members of box
 * j (owned or not) and points owned by it, overwritten for j < h_n_boxes[k], the rest untouched; integer sums, so the
 * result does not depend on the order of arrival.  With both NULL the walk of a point stops at its first hit.
 * d_ws: cv_decode_instances_workspace_bytes(num_cats, max_boxes) bytes.  Asynchronous on `stream`, no host wait; n == 0 is
 * a no-op success.  CV_EINVAL before anything is launched: a NULL grid, points or owner pointer, NULL d_prob with
 * confident_only, n < 0, num_cats outside 1..CV_MAX_CATEGORIES, h_n_boxes[k] outside 0..max_boxes, a cell outside
 * [0, X*Y*Z), a workspace that is too small. */
size_t cv_decode_instances_workspace_bytes(int num_cats, int max_boxes);
int cv_decode_instances_f32(const float* d_grid_rot, const float* d_grid_scale, const int dims[3],
                            const float h_corner3[3], float res, const float* d_points, const float* d_prob, int64_t n,
                            int num_cats, const int64_t* h_cells, const int32_t* h_label_of, const int* h_n_boxes, int max_boxes,
                            float prob_thresh, int confident_only, int32_t* d_owner, int32_t* d_count_in, int32_t* d_count_owned,
                            void* d_ws, size_t ws_bytes, void* stream);

/* utils/calc_map.py:6-21 on two [8][3] corner sets (host). */
double cv_iou_obb(const float* h_box1, const float* h_box2);
/* eval_joint.py:75-89 (host): greedy NMS, returns the pick count, indices in h_pick. */
int cv_nms_obb(const float* h_boxes, const float* h_scores, int n, double thr, int32_t* h_pick);

/* ------------------------------------------------------------------------ *
 * Sparse-voxel engine: replaces the MinkowskiEngine v0.5.3 calls of the network
 * (external dependency, README.md:53; call sites utils/minkunet.py:53-180,
 * utils/resnet.py:118-154, train_joint.py:250, eval_joint.py:169-171).
 * Coordinates are int32 [n][4] = (batch, x, y, z), features fp32 row-major with an
 * explicit leading dimension, weights are ME's `kernel` layout [K^3][Cin][Cout]
 * ([Cin][Cout] for 1x1), kernel-offset index with the first spatial axis fastest.
 * ------------------------------------------------------------------------ */

/* Hash-table slots needed for a coordinate set of n rows (power of two >= 2n). */
long long cv_sp_table_capacity(long long n);
size_t cv_sp_levels_workspace_bytes(long long n);

/* Coordinate sets of tensor strides 1,2,4,8,16 (ME coordinate manager: stride-2 sets are
 * unique(floor(c / 2ts) * 2ts), ordered by first appearance) and one hash table per level.
 * d_coords[0] is the caller's input (n rows); d_coords[1..], d_keys[L], d_vals[L] are caller
 * allocated (n rows / `cap` slots each).  h_counts[0..4] = rows per level, h_counts[5] = number
 * of duplicate input coordinates (must be 0), h_counts[6] = rows outside the 16-bit key window (spatial
 * coordinates in [-32704, 32703], batch index < 65536; must be 0).  Synchronises `stream` once, or not at all when
 * h_counts is NULL (the counts then stay in d_counts only). */
int cv_sp_build_levels(int32_t* const* d_coords, unsigned long long* const* d_keys,
                       int32_t* const* d_vals, long long n, long long cap, int num_levels,
                       int32_t* d_counts, int32_t* h_counts, void* d_ws, size_t ws_bytes, void* stream);

/* Voxelisation of raw point clouds (ME.utils.sparse_quantize, utils/dataloader.py:197, sunrgbd/brnetcanon.py:218): voxel
 * = floor(p / quantization_size) per component - the correctly rounded quotient in the input's own precision, then floor
 * (what numpy computes; no reciprocal) - or floor(p) when floor_only != 0 (quantization_size is then ignored).  One
 * output row per occupied voxel, in the order of each voxel's FIRST point (np.sort of np.unique's return_index):
 *   d_points  [m][ld] device, the three coordinates in the first columns of a row (ld >= 3, in elements)
 *   h_offsets host array of n_clouds first rows (h_offsets[0] == 0, non-decreasing, <= m) when the rows are n_clouds
 *             clouds one after the other - cloud b's rows get batch index b, 1 <= n_clouds <= CV_QUANTIZE_MAX_CLOUDS - or NULL
 *             (n_clouds ignored): one cloud, batch index 0
 *   d_coords4 [m][4] int32 (batch, x, y, z), the first N rows written      d_index [m] int32, the first N written:
 *             row of the first point of each voxel, ascending              d_inverse [m] int32 or NULL: output row of every
 *             point's voxel (-1 for a rejected point)
 *             d_coords4 must be 16-byte aligned (a row is stored as one 16-byte word), else CV_EINVAL before any launch;
 *             rows behind N, and d_index entries behind N, are left as they were.
 *   d_counts int32[2] device: [0] = N, [1] = rejected points.  A point is rejected - counted, kept out of the table and
 *             of every index computation - when a component is not finite or its voxel lies outside the key window of the
 *             coordinate manager (spatial coordinates in [-32704, 32703]); callers treat [1] != 0 as an error.
 *   h_counts  receives the same two ints (one synchronisation of `stream`), or NULL: no host wait.
 *   d_ws      cv_sp_quantize_workspace_bytes(m) bytes; m <= 2^29.
 * Every reduction is a minimum over row indices or an ordered scan: the outputs are bit-reproducible, whatever the schedule. */
#define CV_QUANTIZE_MAX_CLOUDS 256
size_t cv_sp_quantize_workspace_bytes(long long m);
int cv_sp_quantize_f32(const float* d_points, long long m, long long ld, float quantization_size, int floor_only,
                       const long long* h_offsets, int n_clouds, int32_t* d_coords4, int32_t* d_index, int32_t* d_inverse,
                       int32_t* d_counts, int32_t* h_counts, void* d_ws, size_t ws_bytes, void* stream);
int cv_sp_quantize_f64(const double* d_points, long long m, long long ld, double quantization_size, int floor_only,
                       const long long* h_offsets, int n_clouds, int32_t* d_coords4, int32_t* d_index, int32_t* d_inverse,
                       int32_t* d_counts, int32_t* h_counts, void* d_ws, size_t ws_bytes, void* stream);

/* What a scene needs from the voxeliser's outputs, in ONE launch: the world points of the voxels and up to
 * CV_GATHER_MAX_JOBS row gathers by the first-point index (features, raw-point-aligned predictions, labels).
 *   d_coords4 [n][4], d_index [n]  as cv_sp_quantize_* wrote them (d_coords4 may be NULL without d_points_out, d_index without jobs)
 *   d_points_out [n][3] or NULL    points[i][k] = float(coords4[i][1 + k]) * res: the int32 -> fp32 conversion and ONE fp32
 *                                  multiply by `res` (what the scene calls read as cv_scene_desc.d_points)
 *   jobs [n_jobs]                  host array, carried in the kernel arguments (no device table, no copy):
 *                                  dst[i][0:width] = src[index[i]][0:width], rows of 4-byte words moved as words - fp32 payloads
 *                                  (NaNs included) and int32 values come through bit for bit.  src_ld / dst_ld: row strides in
 *                                  words (>= width; destination words beyond `width` are left alone).  recentre_from >= 0:
 *                                  columns >= recentre_from are fp32 and written as x * 2 - 1 (the colour recentre of
 *                                  eval_joint.py:167-168; x * 2 is exact: one rounding); -1: none.
 * Every argument is validated before the first device call.  Asynchronous on `stream`. */
#define CV_GATHER_MAX_JOBS 8
typedef struct cv_gather_job {
    const void* d_src; long long src_ld;
    void* d_dst; long long dst_ld;
    int width;
    int recentre_from;
} cv_gather_job;
int cv_sp_voxel_rows_f32(const int32_t* d_coords4, const int32_t* d_index, long long n, float res, float* d_points_out,
                         const cv_gather_job* jobs, int n_jobs, void* stream);

/* A TRAINING batch from raw scans, in ONE launch behind the voxeliser: the network's input features and the three label arrays
 * of the n kept rows, computed from the raw per-vertex arrays of the concatenated scans - what
 * ScanNetXYZProbMultiDataset.__getitem__ (utils/dataloader.py:118-210) computes per vertex on the host and then gathers.
 * For kept row i: v = d_index[i] (raw vertex), b = d_coords4[i][0] (cloud), o = d_owner[v] (row of the model table, -1 or
 * outside [0, n_models): background).
 *   feats  colour k: c = (float)((double)rgb[v][k] / 255.0); with a colour table, c = (float)((double)c * colour[b][k]),
 *          c = (float)((double)c + colour[b][3 + k]), c = (float)((double)c + jitter[v]), then clamped to [0, 1] - every
 *          step rounds to fp32, as numpy's in-place `float32 op= float64` does.  use_xyz != 0: the row's three d_points
 *          words come first (width 6, else 3).  recentre != 0: the colour columns are written as c * 2.0f - 1.0f.
 *   xyz    o >= 0: xyz[r] = (float)(((m[r][0] * x + m[r][1] * y) + m[r][2] * z) + m[r][3]) in fp64 with (x, y, z) =
 *          d_points[v] and m = d_minv[o] - this order, no fused multiply-add; background: 0
 *   scale  d_model_scale[o], background 0            cls   d_model_cls[o] widened to int64, background 9
 * d_points [m_points][points_ld] fp32, d_rgb [m_points][3] uint8, d_owner [m_points] int32, d_minv [n_models][3][4] fp64,
 * d_model_scale [n_models][3] fp32, d_model_cls [n_models] int32 (the three may be NULL when n_models == 0),
 * d_colour [n_clouds][6] fp64 (gain, shift) with d_jitter [m_points] fp64 - both or neither.  Destinations are [n][width]
 * windows with row strides in elements (>= width; what lies beyond the width is left alone).
 * Every argument is validated before anything is launched.  No atomics, no host wait; asynchronous on `stream`. */
typedef struct cv_scan_rows_desc {
    const int32_t* d_coords4; const int32_t* d_index; long long n;       /* as cv_sp_quantize_* wrote them; n <= m_points */
    long long m_points;
    const float* d_points; long long points_ld;
    const uint8_t* d_rgb;
    const int32_t* d_owner;
    const double* d_minv; const float* d_model_scale; const int32_t* d_model_cls; int n_models;
    const double* d_colour; const double* d_jitter; int n_clouds;
    int use_xyz, recentre;
    float* d_feats; long long feats_ld;
    float* d_xyz; long long xyz_ld;
    float* d_scale; long long scale_ld;
    long long* d_cls; long long cls_ld;
} cv_scan_rows_desc;
int cv_sp_scan_rows_f32(const cv_scan_rows_desc* desc, void* stream);

/* The coordinate loss of the per-category model (train_separate.py:265-280) over PACKED symmetry labels, and its gradient.
 * A segment is one aligned model of one scan: len_s labelled points, each an output row, and n_pose_s symmetry-equivalent
 * poses with one fp32 target per point and pose.  With w = the component weights,
 *   pose_loss[j]  = sum over the segment's points i and c in 0..2 of w[c] * (out[rows[i]][c] - target[pose][i][c])^2 / (3 len_s)
 *   seg_loss[s]   = min over the segment's poses (on the fp32 pose losses; the LOWEST pose on ties; a NaN pose loss wins, as
 *                   torch.min returns NaN), best[s] = that pose
 *   loss[0]       = xyz_factor * (sum_s seg_loss[s]) / n_segments
 *   grad[row][c] += grad_loss[0] * xyz_factor * 2 * w[c] * (out[row][c] - target[best[s]][i][c]) / (3 len_s n_segments)
 *                   over the labelled points i of the row (a row may belong to several segments)
 * Segments are concatenated: points of segment s are d_rows[d_seg_ptr[s] .. d_seg_ptr[s + 1]), its poses the jobs
 * d_pose_ptr[s] .. d_pose_ptr[s + 1), its targets the block [n_pose_s][len_s][3] that starts at row d_tgt_ptr[s] of
 * d_targets [n_targets][3]; d_pseg[i] = segment of point i.  For the backward, the inverse list: d_urow [n_urows] = the
 * distinct rows ascending, d_upoint[d_uptr[u] .. d_uptr[u + 1]) = the points of row d_urow[u], ascending.
 * Terms and sums are fp64 (fp32 inputs, so every difference is exact), rounded to fp32 once per output.  No atomics: the order
 * of every sum depends on the labels and on cv_sym_loss_chunk_rows() alone, so loss, pose losses, best and gradient are the
 * same bytes on every run and stream.  The gradient goes to the winning pose only: torch's full-reduction min() splits it
 * evenly over exact ties, which distinct poses do not produce.
 * PRECONDITIONS the host cannot see through device pointers: the pointer arrays are prefix sums as described (first entry 0,
 * last entries n_points, n_jobs, n_targets), every segment has at least one point and one pose, and every row lies in
 * [0, n_rows) - the caller checks its largest row on the host before it launches (a row outside reads as NaN and gets no
 * gradient, but nothing else is promised for it).
 * forward:  launches the partial pass and the select pass; writes d_loss [1], d_pose_loss [n_jobs], d_best [n_segments],
 *           d_seg_loss [n_segments]; d_ws: cv_sym_loss_workspace_bytes(n_targets, n_jobs), else CV_ENOMEM (the message names
 *           the size).  n_segments == 0: d_loss[0] = 0 and nothing else is launched.
 * backward: one launch; reads d_best of the forward and d_grad_loss on the device (no host wait) and writes columns 0..2 of
 *           the rows d_urow of d_grad [n_rows][grad_ld], which the caller has zeroed.  n_segments == 0: nothing.
 * Arguments are validated before anything is launched (CV_EINVAL: null pointer, row stride below 3, negative count).
 * Asynchronous on `stream`. */
typedef struct cv_sym_loss_desc {
    const float* d_out; long long n_rows; long long ld;                   /* predictions: columns 0..2 of [n_rows][ld] */
    const int32_t* d_rows; const int32_t* d_pseg; long long n_points;
    const int32_t* d_seg_ptr; const int32_t* d_pose_ptr; const int32_t* d_tgt_ptr; int n_segments; int n_jobs;
    const float* d_targets; long long n_targets;
    const int32_t* d_urow; const int32_t* d_uptr; const int32_t* d_upoint; int n_urows;
    float w[3]; float xyz_factor;
    float* d_loss; float* d_pose_loss; int32_t* d_best; float* d_seg_loss;  /* forward: written; backward: d_best read */
    const float* d_grad_loss; float* d_grad; long long grad_ld;           /* backward only */
    void* d_ws; size_t ws_bytes;                                          /* forward only */
} cv_sym_loss_desc;
int cv_sym_loss_fwd_f32(const cv_sym_loss_desc* desc, void* stream);
int cv_sym_loss_bwd_f32(const cv_sym_loss_desc* desc, void* stream);
size_t cv_sym_loss_workspace_bytes(long long n_targets, int n_jobs);
int cv_sym_loss_chunk_rows(void);           /* rows per workgroup of the partial pass: the chunking the sums are ordered by */

/* The per-row losses of both trainers over the network output d_out [n_rows][ld] fp32 (train_joint.py:253-283 and :311-340,
 * train_separate.py:247-262): the masked squared errors of the chosen head's coordinate and scale columns and the cross
 * entropy of the logit columns.  Per row i with label y = d_labels[i] (int64):
 *   obj     = obj_lo <= y <= obj_hi
 *   head h  = gather LABEL: y on object rows, else 0;  gather ARGMAX: the first maximum of the n_logits logits (fp32 `>`, as
 *             cv_head_joint_f32 compares), the LAST logit mapping to 0 (train_joint.py:315-316);  heads == 1: always 0
 *   e_xyz   = sum_c w[c] * (out[xyz_col + 3 h + c] - xyz_labels[i][c])^2            object rows, with_xyz only
 *   e_scale = sum_c w[c] * (out[scale_col + 3 h + c] - t[c])^2, t = log(scale_labels[i]) with log_scale      object rows
 *   ce      = lse - logit[target], target = y, a NEGATIVE label counting as n_logits - 1; the maximum is subtracted before exp
 * Background rows: predictions and targets are selected away in front of the arithmetic - a NaN or Inf there reaches neither
 * a loss nor a gradient.  A label above n_logits - 1 cannot be seen from the host: it makes loss_class (and that row's logit
 * gradients) NaN and is counted in d_info[1]; nothing aborts.
 *   cnt        = object rows -> d_info[0]
 *   denom      = empty ZERO: max(3 cnt, 1) (a batch without object rows gives zero terms: the training form);
 *                empty NAN: 3 cnt (no object row gives NaN, the reference's mean over nothing: the validation form)
 *   d_losses   = {loss_xyz = xyz_factor * sum e_xyz / denom, loss_scale = scale_factor * sum e_scale / denom,
 *                 loss_class = sum ce / n_rows, total = (loss_scale + loss_xyz) + loss_class in fp32}
 * Terms and sums are fp64 from the fp32 inputs, each output is rounded to fp32 once.  No atomics: a workgroup sums
 * cv_row_loss_chunk_rows() rows in a fixed order and writes four fp64 partials (and its count of labels above n_logits - 1)
 * to the workspace, ONE workgroup adds the partials (each lane a contiguous stretch in order, then a fixed tree over the
 * lanes; any number of partials).  The order depends on n_rows, the column layout and the chunk alone: the same bytes on
 * every run and stream.
 * forward:  two launches; writes d_losses [4] and d_info [2]; d_ws: cv_row_loss_workspace_bytes(n_rows), else CV_ENOMEM (the
 *           message names the size).  n_rows == 0: d_losses = 0 (NaN with empty NAN), d_info = 0, nothing else is launched.
 * backward: gather LABEL only (ARGMAX: CV_EINVAL).  One launch; reads d_grad_loss[0] and d_info[0] (the forward's cnt; lse is
 *           recomputed) on the device and writes EVERY element of columns [0, n_cols) of d_grad [n_rows][grad_ld] exactly
 *           once - the caller zeroes nothing: the chosen head's columns of object rows get
 *           g * factor * 2 * w[c] * (p - t) / denom, the logit columns g * (softmax_k - [k == target]) / n_rows, every other
 *           column an exact 0.  Columns from n_cols on are not touched.
 * Every field is validated before the first device call (CV_EINVAL: null pointer, ld or n_cols below the last used column,
 * overlapping column ranges, negative count, n_rows of 2^31 or more, heads < 1, n_logits < 2 or > 16, obj_lo < 0 or
 * obj_hi >= heads with heads > 1, ARGMAX with n_logits - 1 > heads > 1, more than 8192 words for 16 staged rows).
 * Asynchronous on `stream`. */
#define CV_ROW_LOSS_GATHER_LABEL 0
#define CV_ROW_LOSS_GATHER_ARGMAX 1
#define CV_ROW_LOSS_EMPTY_ZERO 0
#define CV_ROW_LOSS_EMPTY_NAN 1
typedef struct cv_row_loss_desc {
    const float* d_out; long long n_rows; long long ld;
    const int64_t* d_labels;                                      /* [n_rows] */
    const float* d_xyz_labels; const float* d_scale_labels;       /* [n_rows][3] each; d_xyz_labels may be NULL without with_xyz */
    int heads; int n_logits; int xyz_col; int scale_col; int logit_col;
    long long obj_lo; long long obj_hi;                           /* inclusive */
    int with_xyz; int log_scale; int gather; int empty;
    float w[3]; float xyz_factor; float scale_factor;
    float* d_losses; int32_t* d_info;                             /* forward: written [4], [2]; backward: d_info[0] read */
    const float* d_grad_loss; float* d_grad; long long grad_ld; int n_cols;      /* backward only */
    void* d_ws; size_t ws_bytes;                                  /* forward only */
} cv_row_loss_desc;
int cv_row_loss_fwd_f32(const cv_row_loss_desc* desc, void* stream);
int cv_row_loss_bwd_f32(const cv_row_loss_desc* desc, void* stream);
size_t cv_row_loss_workspace_bytes(long long n_rows);
int cv_row_loss_chunk_rows(void);           /* rows per workgroup of the partial pass: the chunking the sums are ordered by */

/* The per-category trainer's batch from raw scans, behind the voxeliser and with NO host wait in front: the packed symmetry
 * labels cv_sym_loss_* consume (data.SymBatch) and the per-row arrays, from raw per-vertex arrays plus per-model vertex
 * lists - what ScanNetXYZProbSymDataset.__getitem__ (utils/dataloader.py:339-476) and data.pack_sym compute on the host.
 * The voxeliser ran with d_inverse and h_counts == NULL; N is read on the device from d_quant_counts[0].
 * Candidates: d_seg_vertex [n_cand] = the vertex lists of the batch's n_seg_in segments (one aligned model of one scan, batch
 * order) one after the other, list s = [d_seg_vptr[s], d_seg_vptr[s + 1]); its poses are the jobs [d_seg_pose_ptr[s],
 * d_seg_pose_ptr[s + 1]) of d_minv [n_jobs_in][3][4] fp64.  Both pointer arrays are prefix sums (first entry 0, last entries
 * n_cand and n_jobs_in) - a precondition, like the vertices lying in [0, m_points) (a vertex outside is dropped).
 *   1 survivors  candidate q with v = seg_vertex[q] survives iff r = inverse[v] >= 0 and index[r] == v (v is the first point
 *                of its voxel).  Kept candidates are compacted by an ordered scan: segment order, list order, duplicates kept.
 *   2 segments   len_s = kept candidates of segment s; segments with len_s == 0 are dropped, the others renumbered in order.
 *                seg_ptr / pose_ptr / tgt_ptr [S + 1] = prefix sums over the kept segments of len, n_pose and len * n_pose;
 *                pseg[p] = new segment of kept point p; rows[p] = r, minus the first row of the point's cloud when
 *                reference_indexing != 0 (rows of a cloud are contiguous: the first row of cloud b is the lower bound of
 *                d_offsets[b] in the ascending d_index).
 *   3 targets    kept segment s, pose j, point i, (x, y, z) = d_points[v], m = d_minv[job]:
 *                targets[tgt_ptr[s] + j * len_s + i][r] = (float)(((m[r][0] * x + m[r][1] * y) + m[r][2] * z) + m[r][3])
 *                in fp64, this order, no fused multiply-add.
 *   4 inverse    urow [U] = the distinct rows ascending, uptr [U + 1] their prefix, upoint [P] the points of each row in
 *                ascending point index (np.argsort(rows, kind="stable") / np.unique(rows, return_counts=True)).  Rows are
 *                counted with integer atomics, a row's points are placed by an atomic slot and then SORTED by one lane per
 *                row (insertion sort: quadratic in the multiplicity of a row, meant for the handful of overlapping models
 *                and scans that share a row).
 *   5 rows       for the N kept rows, v = index[i], b = coords4[i][0], o = owner[v] (outside [0, n_models): background):
 *                colour k without d_colour: c = (float)((double)rgb[v][k] / 255.0); with d_colour [n_clouds][6] (gain, shift)
 *                and d_jitter [m_points]: t = (double)rgb[v][k]; t = t * gain[b][k]; t = t + shift[b][k]; t = t + jitter[v];
 *                t = min(max(t, 0), 1); c = (float)(t / 255.0) - fp64 throughout, one rounding.  recentre != 0: c * 2.0f -
 *                1.0f.  use_xyz != 0: the row's three d_points words first (width 6, else 3).  scale = d_model_scale[o] or 0,
 *                obj = (o >= 0) and cls = d_model_cls[o] or 0, both int64.
 *   6 counts     d_counts int32[8] = P, S, J, T, U, max_row (urow[U - 1], -1 when U == 0), N, rejected points - and the same
 *                eight ints to h_counts (PINNED host memory, or NULL) by a copy on the stream; valid once the stream's work
 *                up to this call has completed.  Without a kept segment S = P = J = T = U = 0 and max_row = -1; the row
 *                arrays are still written.
 * Output buffers hold the host's upper bounds: rows / pseg / urow / upoint [n_cand], uptr [n_cand + 1], seg_ptr / pose_ptr /
 * tgt_ptr [n_seg_in + 1], targets [n_targets_in][3] with n_targets_in >= sum of list length * n_pose, the row arrays
 * [m_points] rows (strides in elements).  Only the counted prefixes are written.  Arrays of a zero bound may be NULL.
 * d_ws: cv_sp_sym_rows_workspace_bytes(m_points, n_cand, n_seg_in, n_clouds), else CV_ENOMEM.
 * Every sum is an ordered scan or an integer count: the outputs are the same bytes on every run and stream.
 * Every argument is validated before anything is launched.  No host wait; asynchronous on `stream`. */
typedef struct cv_sym_rows_desc {
    const int32_t* d_coords4; const int32_t* d_index; const int32_t* d_inverse;   /* as cv_sp_quantize_* wrote them, [m_points] rows */
    const int32_t* d_quant_counts;                                                  /* its d_counts: [0] = N, [1] = rejected */
    long long m_points;
    const float* d_points; long long points_ld;
    const uint8_t* d_rgb;
    const int32_t* d_owner;
    const float* d_model_scale; const int32_t* d_model_cls; int n_models;
    const double* d_colour; const double* d_jitter;
    const long long* d_offsets; int n_clouds;                                       /* device: first vertex of every cloud */
    const int32_t* d_seg_vertex; long long n_cand;
    const int32_t* d_seg_vptr; const int32_t* d_seg_pose_ptr; int n_seg_in;
    const double* d_minv; long long n_jobs_in;
    long long n_targets_in;
    int reference_indexing, use_xyz, recentre;
    int32_t* d_rows; int32_t* d_pseg; int32_t* d_seg_ptr; int32_t* d_pose_ptr; int32_t* d_tgt_ptr; float* d_targets;
    int32_t* d_urow; int32_t* d_uptr; int32_t* d_upoint;
    float* d_feats; long long feats_ld;
    float* d_scale; long long scale_ld;
    long long* d_obj; long long* d_cls;
    int32_t* d_counts; int32_t* h_counts;
    void* d_ws; size_t ws_bytes;
} cv_sym_rows_desc;
int cv_sp_sym_rows_f32(const cv_sym_rows_desc* desc, void* stream);
size_t cv_sp_sym_rows_workspace_bytes(long long m_points, long long n_cand, int n_seg_in, int n_clouds);
int cv_sp_sym_rows_block(void);             /* candidates per workgroup of the candidate passes (first level of their scan) */
long long cv_sp_sym_rows_scan_span(void);   /* candidates one trip of the second scan level covers: beyond it, a second trip */

/* Spatial row order of a coordinate set (what the fused network runs on; replaces the sort of Morton keys by the
 * caller): stable sort on (batch index, Z-order of the 2^shift cubes), rows of one cube in the caller's order.
 * d_sorted[n][4] = rows in that order, d_perm[n] = original row of each sorted row, d_inv[n] = sorted row of each
 * original row.  d_ws: cv_sp_sort_workspace_bytes(n).  Asynchronous, no host synchronisation. */
size_t cv_sp_sort_workspace_bytes(long long n);
int cv_sp_sort_rows(const int32_t* d_coords, long long n, int32_t* d_sorted, int32_t* d_perm, int32_t* d_inv,
                    void* d_ws, size_t ws_bytes, void* stream);

/* Z-order (Morton) sort keys, batch index in the top bits: d_keys[n] int64.  Asynchronous. */
int cv_sp_morton_keys(const int32_t* d_coords, long long n, long long* d_keys, void* stream);

/* Kernel map of a k^3 kernel (ME "kernel map" / neighbour table): d_nbr[n_out][k^3] = input row of
 * out_coord + offset*ts or -1.  Odd k centred, even k offsets 0..k-1.  Asynchronous. */
int cv_sp_kernel_map(const int32_t* d_out_coords, long long n_out, const unsigned long long* d_keys,
                     const int32_t* d_vals, long long cap, int k, int ts, int32_t* d_nbr, void* stream);

/* Map of MinkowskiConvolutionTranspose(kernel_size=2, stride=2) onto the existing finer set,
 * derived from the matching strided map: d_up[n_fine][8]. */
int cv_sp_up_map(const int32_t* d_nbr_down, long long n_coarse, long long n_fine, int32_t* d_up,
                 void* stream);

/* out[u][:] = relu?( (acc_in[u][:] + sum_{j in [j_begin,j_end)} W_j^T in[nbr[u][j]]) * scale + shift
 *                    + residual[u][:] )
 * = MinkowskiConvolution / ConvolutionTranspose with the eval-mode MinkowskiBatchNorm, bias,
 * BasicBlock residual and MinkowskiReLU folded into the epilogue.  Optional members may be NULL / 0. */
typedef struct cv_conv_desc {
    const float* in;        /* [n_in][in_ld] input features */
    long long n_in;
    int in_ld, cin;
    const float* weight;    /* [K][cin][cout] (ME `kernel`) */
    int K, cout;
    const int32_t* nbr;     /* [n_out][K] kernel map; NULL for K == 1 on the same coordinate set */
    long long n_out;
    const float* scale;     /* [cout] or NULL */
    const float* shift;     /* [cout] or NULL */
    const float* residual;  /* [n_out][res_ld] or NULL */
    int res_ld;
    int relu;
    float* out;             /* [n_out][out_ld] */
    int out_ld;
    int flavour;            /* 0 auto (may split offsets over workgroups through ws), 1 never split */
    void* ws;               /* optional workspace, cv_sp_conv_workspace_bytes */
    size_t ws_bytes;
    const int32_t* row_perm;/* optional [n_out] processing order (rows with equal neighbour masks adjacent) */
    int j_begin, j_end;     /* kernel offsets to accumulate; j_end == 0 means K */
    const float* acc_in;    /* optional [n_out][acc_ld] partial sums from a previous launch */
    int acc_ld;
    int perm_groups;        /* >1: row_perm is [perm_groups][n_out]; the offsets are split into that many
                               contiguous groups, each run in its own order in ONE launch (needs ws) */
    const int32_t* plan_ent;/* reserved, must be NULL (round 1-3: the pair lists of an experimental tile kernel, removed) */
    const int32_t* plan_cnt;/* reserved, must be NULL */
    const float* weight_packed; /* reserved, must be NULL */
    const void* weight_x6;  /* optional: the same weights from cv_sp_pack_weights_x6_f32.  When given (and Cin % 32 == 0)
                               the products run on the bf16 matrix cores as six bf16 x bf16 piece products per fp32
                               product (fp32-level accuracy, 0.375x the matrix time of v_mfma_f32_32x32x2_f32) */
    const float* in2;       /* optional second source on the OUTPUT rows (bf16x6 path only): the accumulator also gets */
    int in2_ld, cin2;       /* in2[u][0:cin2] @ W2 - BasicBlock's 1x1 downsample branch folded into conv2             */
    const void* weight2_x6; /* cv_sp_pack_weights_x6_f32 of W2 [1][cin2][cout] (the packer of weight_pieces, as weight_x6).
                               At most 28 kernel offsets per workgroup: a launch that does not split below that (flavour 1,
                               or flavour 0 without ws, with more than 28 offsets in [j_begin, j_end)) is CV_EINVAL - the
                               kernel that takes such launches has no second source                                  */
    int perm_has_map;       /* with perm_groups > 1: row_perm is followed by the kernel map rows in processing order
                               (cv_sp_mask_perms with_map = 1), which turns the random map reads into coalesced ones */
    int weight_pieces;      /* 1: one bf16 plane (cv_sp_pack_weights_bf16_f32): operands rounded to bf16, one product -
                               the opt-in bf16 compute mode, NOT fp32-level accuracy;
                               0 / 3: weight_x6 (and weight2_x6) hold bf16 triples (cv_sp_pack_weights_x6_f32);
                               2: fp16 pairs (cv_sp_pack_weights_h2_f32): three fp16 x fp16 piece products per fp32
                               product - fp32-level accuracy (operands to 2^-24) while every input magnitude is below
                               65504, half the matrix time of the triples                                            */
    float acc_scale;        /* fp16 pairs: 2^-scale_log2 of the pack call (0 = 1): multiplies the accumulators        */
    int32_t* range_flag;    /* fp16 pairs: optional device-visible word, set to 1 when an input magnitude > 65000 was
                               staged (the result is then invalid: redo the convolution with the bf16 triples)        */
    int in_hl, out_hl, res_hl; /* 1: in (and in2) / out / residual are in the hl format instead of fp32 - the fp16 pair
                               (h, l) of every value stored in place: a row of C channels (C % 32 == 0) keeps its 4*C
                               bytes, each 32-channel chunk = 64 bytes of high pieces then 64 bytes of low pieces
                               (cv_sp_to_hl_f32 / cv_sp_from_hl_f32).  The consumer then loads its matrix-core operand
                               fragments straight from global memory and nothing is split per gather; the producer
                               raises range_flag when an OUTPUT magnitude exceeds 65000.  Needs weight_pieces = 2 for
                               in_hl, channel counts and leading dimensions % 32 == 0, 128-byte aligned rows.        */
    int32_t* split_tickets; /* optional, hl-format input only: CV_SPLIT_TICKETS zero-initialised ints owned by the caller's
                               stream.  A split launch then reduces its partial tiles in the last-arriving workgroup of every
                               output tile (same summation order as the finish launch: bit-identical) instead of a second
                               launch; the library leaves the counters at zero.  NULL: two launches. */
    const float* acc_scale_dev; /* optional, hl-format input only: a device scalar multiplied into acc_scale when the kernel
                               runs (the training backward scales a layer's gradient rows by a power of two chosen on the
                               device, cv_sp_bn_backward_hl_f32, and hands the inverse over here: no host wait). */
    const int32_t* valid_words; /* optional, with perm_has_map and K <= 32: [n_out] validity word of every row of nbr, bit j =
                               nbr[row][j] >= 0 (the scene plan leaves one behind each 3x3x3 map).  Read only under option
                               "zskip": (group, row) pairs without a neighbour then cost no partial tile.  NULL: as before. */
} cv_conv_desc;
#define CV_SPLIT_TICKETS 4096

/* fp32 rows -> hl format and back (d_x and d_y may not alias; c % 32 == 0; the hl side 128-byte aligned with a leading
 * dimension % 32 == 0; leading dimensions in 4-byte units on both sides).  range_flag (optional) as in cv_conv_desc. */
int cv_sp_to_hl_f32(const float* d_x, long long n, int c, int x_ld, float* d_y, int y_ld, int32_t* range_flag, void* stream);
int cv_sp_from_hl_f32(const float* d_x, long long n, int c, int x_ld, float* d_y, int y_ld, void* stream);

/* Weights of the bf16x6 path: [K][cin][cout] fp32 split into three bf16 pieces per value (h + m + l == value to half
 * an fp32 ulp), laid out per (offset, 32-channel chunk) as [piece][cout][32]: 3*K*cin*cout 16-bit words, 16-byte aligned;
 * cin % 32 == 0; redo whenever the weights change.  Asynchronous. */
int cv_sp_pack_weights_x6_f32(const float* d_w, int K, int cin, int cout, const float* d_col_scale, void* d_wp6,
                              void* stream);   /* d_col_scale[cout] (optional): weights are multiplied per output
                                                  column before the split (a folded BatchNorm scale) */
/* Weights of the fp16-pair path: (w * d_col_scale * 2^scale_log2) split into h + l fp16 pieces, same layout with two
 * planes: 2*K*cin*cout 16-bit words.  The caller picks scale_log2 (largest scaled magnitude about 2^13; both weight
 * sets of a two-source convolution share it) and passes acc_scale = 2^-scale_log2 in the descriptor. */
int cv_sp_pack_weights_h2_f32(const float* d_w, int K, int cin, int cout, const float* d_col_scale, int scale_log2,
                              void* d_wp, void* stream);
/* cv_sp_pack_weights_h2_f32 / cv_sp_pack_weights_t_f32 (pieces 2) for MANY weight tensors in ONE launch: a training step packs
 * the fp16 pairs of all 63 convolutions - forward and transposed - in front of its forward instead of one launch per layer
 * and direction (117 launches and the stream's idle time in front of them, profiles/r5/train_gaps.txt).  Job i packs
 * w[K][cin][cout] (trans = 0) or, trans = 1, the transposed convolution of a FORWARD kernel w[K][cout][cin] (what
 * cv_sp_pack_weights_t_f32(w, K, rows = cout, cols = cin, 2, ...) makes) into wp: 2*K*cin*cout 16-bit words, 16-byte
 * aligned, no column scale.  h_jobs: host array, copied to d_jobs by hipMemcpyAsync on `stream`: ordinary (pageable) memory is
 * staged before the call returns and may be reused at once; a PINNED array is read when the copy runs on the stream and must stay
 * unchanged until then.  d_jobs: n_jobs * sizeof(cv_pack_job) bytes of device scratch that must stay untouched until the launch
 * has run. */
typedef struct cv_pack_job {
    const float* w;
    void* wp;
    int K, cin, cout;
    int trans;
    int scale_log2;
    int reserved;
} cv_pack_job;
int cv_sp_pack_weights_h2_batch_f32(const cv_pack_job* h_jobs, int n_jobs, void* d_jobs, void* stream);
/* Weights of the opt-in bf16 compute mode (cv_conv_desc.weight_pieces = 1): w * d_col_scale rounded to bf16 (RNE),
 * one plane of the same layout: K*cin*cout 16-bit words.  Not an fp32-parity path (operands carry 8 significant
 * bits); the reference trains and evaluates in fp32 (train_joint.py:218), BASELINE config 3 asks for bf16. */
int cv_sp_pack_weights_bf16_f32(const float* d_w, int K, int cin, int cout, const float* d_col_scale, void* d_wp,
                                void* stream);
/* Packed weights of the TRANSPOSED convolution (the input gradient of a layer: the same kernel on the transposed map with
 * W_j^T) straight from the layer's forward weights d_w[K][rows][cols]: what cv_sp_pack_weights_{x6,h2,bf16}_f32 would make
 * of W'[K][cols][rows], W'[j][a][b] = d_w[j][b][a], without materialising W'.  cols % 32 == 0.  pieces: 3 bf16 triples,
 * 2 fp16 pairs (times 2^scale_log2), 1 one bf16 plane. */
int cv_sp_pack_weights_t_f32(const float* d_w, int K, int rows, int cols, int pieces, int scale_log2, void* d_wp, void* stream);
/* Weights of the matrix-core stem (Cin 3 or 6 -> 32 channels, K <= 128 offsets; cv_conv_desc with weight_pieces = 2 and
 * this buffer in weight_x6): (w * d_col_scale * 2^scale_log2) as fp16 pairs in MFMA B-operand order, 8 * cin * 2048 bytes;
 * pass acc_scale = 2^-scale_log2 and no `scale` in the descriptor. */
int cv_sp_pack_weights_stem_h2_f32(const float* d_w, int K, int cin, const float* d_col_scale, int scale_log2, void* d_wp,
                                   void* stream);

size_t cv_sp_conv_workspace_bytes(long long n_out, int cout, int K);
int cv_sp_conv_f32(const cv_conv_desc* desc, void* stream);

/* Launch sizing of the convolutions whose output tiles alone do not fill the chip (the coarse levels): the number of
 * workgroups a launch is split up to (over the kernel offsets; partial tiles, then a finish pass).  Default 768
 * (or CV_SPLIT_TARGET) - best for ONE scene in flight; a host that keeps several scenes in flight on separate streams
 * lets the other scenes fill the chip and sets a smaller value (bench.py: 256 from four scenes in flight).  Results
 * change in the summation order only (fp32 rounding).  workgroups <= 0 restores the default.  Returns the previous
 * value.  Process-wide; set it before launching, not concurrently with cv_sp_conv_f32 / cv_sp_net_forward callers that
 * need one fixed value.  (No reference counterpart: MinkowskiEngine's launch sizes are internal.) */
int cv_sp_set_split_target(int workgroups);
/* The same for the CALLING THREAD's launches only (0 = follow the process-wide value); returns the previous thread value.
 * cv_detect_scene_f32 uses it to size a scene's launches by how many scenes are in flight when it starts. */
int cv_sp_set_split_target_thread(int workgroups);
/* Measurement hook (no reference counterpart; results are WRONG while a bit is set): timing ablations that can be switched
 * at run time, after a warm-up has filled every buffer with valid values.  bit 0: the finish launches of the split / mask-group
 * convolutions are skipped (what the partial-tile reductions cost with scenes in flight).  Returns the previous bits. */
int cv_sp_set_ablation(int bits);
/* Kernel selection knobs of cv_sp_conv_f32 / cv_net_run_f32 (process-wide, like cv_sp_set_split_target; results are
 * bit-identical under every setting).  "hd_mask": bit NB - 1 sends the hl-format convolutions whose workgroups are
 * NB x 32 columns wide to conv_hd (LDS-DMA operand rings, 256-row workgroups) instead of conv_hl when the launch has at
 * least "hd_min_rows" output rows; "hd_shape": 0 = 8 waves x 3 ring stages (one workgroup per CU), 1 = 4 waves x 2 stages
 * (two per CU), 2 = 8 waves x 2 stages.  "zskip" (CV_ZSKIP, default 0): mask-sorted hl convolutions whose descriptor carries
 * cv_conv_desc.valid_words write and read no partial tile for (group, row) pairs without a neighbour; the scene calls pass
 * their plan's words, cv_net_run_f32 / cv_net_run_models_f32 pass none (the knob does nothing there).  "zskip_launches": not
 * a knob but a counter - convolutions dispatched with validity words so far; set it to reset it.
 * *previous (may be NULL) receives the old value.  Environment defaults: CV_HD, CV_HD_MIN_ROWS, CV_HD_SHAPE, CV_ZSKIP. */
int cv_sp_set_option(const char* name, long long value, long long* previous);
/* Reads a knob of cv_sp_set_option without touching it (other threads may be launching). */
int cv_sp_get_option(const char* name, long long* value);

/* Every kernel map and processing order the fused MinkUNet forward needs, built by ONE call per scene into one
 * int32 arena (offsets in int32 words; -1 = absent):
 * (level-0 items first - stem, k3[0], mask_perm[0], scratch - then the coarse levels)
 *   stem  [rows0][stem_k^3]  sorted rows <- rows of the caller's order (the sorted set's own map with d_perm, the
 *                            sorted <- original permutation of cv_sp_sort_rows, folded in)
 *   out                      always -1: the caller's rows <- sorted rows map is cv_sp_sort_rows' d_inv
 *   down[i] [rows(i+1)][8]   k2s2 conv level i -> i+1;   k3[i] [rows(i)][27];   up[i] [rows(3-i)][8] level 4-i -> 3-i
 *                            (behind k3[i]: rows(i) validity words, bit j = k3[i][row][j] >= 0, at k3[i] + 27 * rows(i);
 *                            written for level 0 and for the levels that have a mask_perm)
 *   mask_perm[i] [groups][rows(i)] for levels with >= masked_min_rows rows;  up_perm[i] [rows(3-i)] octant order
 * d_coords / d_keys / d_vals: the five levels of the (Z-order sorted) coordinate set from cv_sp_build_levels. */
typedef struct cv_scene_maps {
    long long stem, out, down[4], k3[5], up[4], mask_perm[5], up_perm[4], scratch;
    long long bitmap;       /* 2^20 words: occupancy bits of the level-0 set over its bounding box (cv_sp_scene_plan puts
                               them in front of the hash probes of the level-0 maps: 87 % of the lookups are misses) */
} cv_scene_maps;
size_t cv_sp_scene_maps_words(const long long* level_rows, long long n_orig, int stem_k, int mask_groups,
                              long long masked_min_rows, cv_scene_maps* offsets);
int cv_sp_scene_maps(int32_t* const* d_coords, const unsigned long long* const* d_keys, const int32_t* const* d_vals,
                     long long cap, const long long* level_rows, const int32_t* d_perm, long long n_orig, int stem_k,
                     int mask_groups, long long masked_min_rows, int32_t* d_arena, size_t arena_words, void* stream);

/* The whole coordinate plan of a scene in ONE call (replaces cv_sp_sort_rows + cv_sp_build_levels + cv_sp_scene_maps
 * issued by the caller): spatial row sort of d_input[n][4] into d_coords[0], the five levels with their tables, every
 * kernel map and processing order of the fused network into d_arena.  The arena is sized before the coarse row counts are
 * known (cv_sp_scene_plan_words: every level bounded by n); *offsets and h_counts[8] (cv_sp_build_levels' counts) are
 * filled on return.  The level counts are copied to pinned host memory behind the levels and the call waits for that copy
 * only (an event), while `stream` goes on with the level-0 maps queued behind it.  When h_counts[5] (duplicates) or h_counts[6] (rows
 * outside the key window) is non-zero nothing beyond the level-0 maps is built and the caller must reject the input. */
size_t cv_sp_scene_plan_words(long long n, int stem_k, int mask_groups, long long masked_min_rows);
int cv_sp_scene_plan(const int32_t* d_input, long long n, int32_t* d_perm, int32_t* d_inv, int32_t* const* d_coords,
                     unsigned long long* const* d_keys, int32_t* const* d_vals, long long cap, int32_t* d_counts,
                     int32_t* h_counts, int stem_k, int mask_groups, long long masked_min_rows, int32_t* d_arena,
                     size_t arena_words, cv_scene_maps* offsets, void* d_sort_ws, size_t sort_ws_bytes, void* d_levels_ws,
                     size_t levels_ws_bytes, void* stream);

/* THE definition of the buffers a scene plan lives in (pure host functions; cv_detect_scene_f32, cv_detect_scene_separate_f32
 * and the Python coordinate manager all take them from here).  One int32 buffer of int_words words holds, at these word
 * offsets (each span rounded up to 64 words, `counts` 64 words): perm [n] | inv [n] | coords[i] [n][4] | vals[i] [cap] |
 * counts [8] | arena (cv_sp_scene_plan_words: every coarse level bounded by n); one 64-bit buffer of key_words words holds
 * the five tables' keys, table i at i * cap. */
typedef struct cv_scene_plan_layout {
    long long cap;                                      /* cv_sp_table_capacity(n) */
    long long perm, inv, coords[5], vals[5], counts, arena;
    long long int_words, key_words;
    size_t sort_ws_bytes, levels_ws_bytes;              /* cv_sp_sort_workspace_bytes(n), cv_sp_levels_workspace_bytes(n) */
} cv_scene_plan_layout;
int cv_sp_scene_plan_layout(long long n, int stem_k, int mask_groups, long long masked_min_rows, cv_scene_plan_layout* out);
/* The pointer tables of cv_net_run_f32 for a plan in d_ibuf: maps = [stem, down 0-3, k3 0-4, up 0-3, out (= inv)], perms =
 * [mask orders of levels 0-4, octant orders of the four transposed convs]; a mask order is NULL where the plan has none or
 * the level has fewer than min_rows rows. */
#define CV_NET_MAP_SLOTS 15
#define CV_NET_PERM_SLOTS 9
int cv_sp_scene_plan_slots(const cv_scene_plan_layout* layout, const cv_scene_maps* offsets, const long long* level_rows,
                           long long min_rows, const int32_t* d_ibuf, const int32_t** maps, const int32_t** perms);
/* cv_net_run_f32's d_ws for the five levels: the partial sums of the mask-sorted levels (masked[i] != 0) and the split-K
 * workspace of the others (cv_sp_conv_workspace_bytes at the largest row count that still splits). */
size_t cv_sp_scene_conv_workspace_bytes(const long long* level_rows, const int* masked, int mask_groups, int max_channels);

/* Fused eval-mode network as ONE call per scene (host-side executor over cv_sp_conv_f32; replaces the reference's
 * module-by-module MinkUNet34C.forward, utils/minkunet.py:122-180, for inference).  The program is symbolic and built
 * once per model: feature buffers are slots of a per-scene arena, kernel maps / processing orders are slots of
 * per-scene pointer tables.
 *   cv_net_buf: level >= 0: arena buffer of level_rows[level] x channels floats;
 *               level < 0: the caller's tensor - takes the next entry of ext_ptr / ext_ld, rows = level_rows[rows_level].
 *   cv_net_op:  out[:, out_col:out_col+cout] = relu?( conv(in[:, in_col:in_col+cin]) * scale + shift
 *               + res[:, res_col:res_col+cout] ), kernel map maps[map] (map < 0: K == 1), processing order
 *               perms[perm] (perm < 0 or a NULL table entry: natural order; perm_groups > 1: mask-sorted groups). */
typedef struct cv_net_buf {
    int level, channels, rows_level;
    int hl;                    /* 1: the buffer holds the hl format (cv_conv_desc.in_hl): every op reading / writing it runs
                                  with the matching flag; arena buffers only */
} cv_net_buf;
typedef struct cv_net_op {
    int in_buf, in_col, cin;
    int out_buf, out_col, cout;
    int res_buf, res_col;      /* res_buf < 0: no residual */
    int map, K;
    int perm, perm_groups;
    int relu;
    const float* weight;       /* [K][cin][cout] */
    const float* scale;        /* [cout] or NULL */
    const float* shift;        /* [cout] or NULL */
    const void* weight_x6;     /* cv_sp_pack_weights_x6_f32 of weight, or NULL */
    int in2_buf, in2_col, cin2;/* second source (in2_buf < 0: none), see cv_conv_desc.in2 */
    const void* weight2_x6;
    int weight_pieces;         /* see cv_conv_desc.weight_pieces / acc_scale */
    float acc_scale;
} cv_net_op;
size_t cv_net_arena_bytes(const cv_net_buf* bufs, int n_bufs, const long long* level_rows, int n_levels);
int cv_net_run_f32(const cv_net_op* ops, int n_ops, const cv_net_buf* bufs, int n_bufs, const long long* level_rows,
                   int n_levels, void* d_arena, size_t arena_bytes, const void* const* ext_ptr, const int* ext_ld,
                   const int32_t* const* maps, int n_maps, const int32_t* const* perms, int n_perms,
                   void* d_ws, size_t ws_bytes, int32_t* range_flag, void* stream);   /* range_flag: cv_conv_desc.range_flag of every fp16-pair op, or NULL */

/* K structurally identical programs (the per-category models of separate mode: same ops, buffers, maps and orders; only
 * the weight / scale / shift pointers, acc_scale and the output tensor differ) as ONE launch sequence: every op is issued
 * once, the model is a launch coordinate of the convolution, finish and stem kernels.  Per model the split counts, mask
 * groups, unit order and summation order are those of cv_net_run_f32: model m's output is bit for bit what cv_net_run_f32
 * gives for program m.  fp16-pair programs on hl buffers only (weight_pieces == 2); anything else is CV_EINVAL.
 *   d_params   device table of cv_net_model_params, what has no constant stride between models: op k's parameters of the K
 *              models at d_params[k * params_ld + m] (params_ld >= K: a pass over models m0 ... of a larger set hands over
 *              table + m0 and the set's size).  Built once per model set: cv_net_models_params_fill writes the host image
 *              [n_ops][K] (cv_net_models_params_bytes), the caller copies it to the device.
 *   d_arena    K arenas, cv_net_models_arena_bytes (= K x cv_net_arena_bytes); model m at m x cv_net_arena_bytes
 *   d_ws       K convolution workspaces, cv_net_models_workspace_bytes of ONE model's size (what cv_net_run_f32 takes):
 *              model m at m x that size rounded up to 256 bytes
 *   ext_ptr    [K] pointer tables as cv_net_run_f32's (ext_ld is shared).  A buffer the program only reads (the input
 *              features) must be the same tensor for every model; the one it writes is model m's own.
 *   range_flag K words 16 ints apart (model m: range_flag + 16 m), or NULL
 * The programs are compared on the host first: n_ops, n_bufs and every integer field of every op and buffer must agree and
 * a pointer may be NULL in all models or in none, otherwise CV_EINVAL names the first differing op and model.
 * 1 <= K <= CV_MAX_CATEGORIES.  Not available with models: cv_conv_desc.split_tickets. */
typedef struct cv_net_model_params {
    const void* weight_x6;     /* cv_net_op.weight_x6 of the model */
    const void* weight2_x6;
    const float* scale;
    const float* shift;
    float acc_scale;
    int reserved[3];
} cv_net_model_params;
size_t cv_net_models_params_bytes(int n_ops, int K);
int cv_net_models_params_fill(const cv_net_op* const* ops, int n_ops, int K, void* h_params, size_t params_bytes);
size_t cv_net_models_arena_bytes(const cv_net_buf* bufs, int n_bufs, const long long* level_rows, int n_levels, int K);
size_t cv_net_models_workspace_bytes(size_t one_model_bytes, int K);
int cv_net_run_models_f32(const cv_net_op* const* ops, const cv_net_buf* const* bufs, int n_ops, int n_bufs, int K,
                          const long long* level_rows, int n_levels, void* d_arena, size_t arena_bytes,
                          const void* const* const* ext_ptr, const int* ext_ld, const int32_t* const* maps, int n_maps,
                          const int32_t* const* perms, int n_perms, void* d_ws, size_t ws_bytes, int32_t* range_flag,
                          const void* d_params, int params_ld, void* stream);

/* d_keys[n] (int64) = bit mask of the valid neighbours among offsets [j_begin, j_end) of every row of a
 * kernel map; argsort of it is a row_perm for cv_conv_desc.  Asynchronous. */
int cv_sp_mask_keys(const int32_t* d_nbr, long long n, int K, int j_begin, int j_end, long long* d_keys,
                    void* stream);

/* d_perm[groups][n]: for each contiguous group of the K kernel offsets, the rows ordered by the bit
 * mask of their valid neighbours in that group (counting sort; at most 10 offsets per group).
 * d_ws: groups * 4096 bytes.  with_map = 1: d_perm holds groups*n*(1 + W) + ceil(groups*n/4) words, W = ceil(K/groups); after the
 * orders come the kernel map rows of every group in processing order, [groups][n][W]
 * (cv_conv_desc.perm_has_map).  Asynchronous. */
int cv_sp_mask_perms(const int32_t* d_nbr, long long n, int K, int groups, int32_t* d_perm, void* d_ws,
                     size_t ws_bytes, int with_map, void* stream);

/* Training support (train_joint.py:283 `loss.backward()` through the sparse convolutions).
 * Input gradient = cv_sp_conv_f32 on the transposed map with the transposed weights:
 *   d_nbr_t[n_in][K], nbr_t[i][j] = u iff nbr[u][j] == i.
 * Weight gradient dW[j][ci][co] = sum_u x[nbr[u][j]][ci] * dy[u][co] (fp32 matrix cores, split over rows). */
int cv_sp_transpose_map(const int32_t* d_nbr, long long n_out, int K, long long n_in, int32_t* d_nbr_t, void* stream);
size_t cv_sp_wgrad_workspace_bytes(long long n_out, int cin, int cout, int K);
int cv_sp_conv_wgrad_f32(const float* d_x, int x_ld, int cin, const float* d_dy, int dy_ld, int cout,
                         const int32_t* d_nbr, int K, long long n_out, float* d_dw, void* d_ws, size_t ws_bytes,
                         void* stream);
/* The same with the product precision chosen by the caller: pieces = 0 fp32 matrix cores, 3 six bf16 piece products
 * per fp32 product (fp32-level accuracy; what cv_sp_conv_wgrad_f32 runs), 1 operands rounded to bf16 and ONE
 * bf16 x bf16 product with fp32 accumulation (the opt-in bf16 compute mode, BASELINE configs 3-4). */
int cv_sp_conv_wgrad_px_f32(const float* d_x, int x_ld, int cin, const float* d_dy, int dy_ld, int cout,
                            const int32_t* d_nbr, int K, long long n_out, float* d_dw, void* d_ws, size_t ws_bytes,
                            int pieces, void* stream);
/* out[c] = sum over rows of x[:, c] (bias gradient).  cv_sp_col_sum_f32 joins the row chunks through fp32 atomics: the
 * last bit depends on the order in which workgroups arrive.  cv_sp_col_sum_det_f32 writes the chunk sums to a workspace
 * (cv_sp_col_sum_workspace_bytes) and adds them in chunk order: the same bits on every run (what the training path uses,
 * so that a train_joint.py step is reproducible bit for bit). */
int cv_sp_col_sum_f32(const float* d_x, long long n, int c, int ld, float* d_out, void* stream);
size_t cv_sp_col_sum_workspace_bytes(long long n, int c);
int cv_sp_col_sum_det_f32(const float* d_x, long long n, int c, int ld, float* d_out, void* d_ws, size_t ws_bytes,
                          void* stream);

/* Training-mode MinkowskiBatchNorm (= nn.BatchNorm1d over the feature rows, utils/minkunet.py:56):
 * batch mean / biased variance per channel, running statistics updated in place (NULL to skip), folded
 * scale/shift for cv_sp_affine_f32; and its backward (d_y = output of the ReLU that follows, or NULL;
 * d_dres = optional ReLU-masked gradient for a residual added before that ReLU, resnet_block forward). */
size_t cv_sp_bn_workspace_bytes(int c);
int cv_sp_bn_stats_f32(const float* d_x, long long n, int c, int ld, const float* d_gamma, const float* d_beta,
                       float eps, float momentum, float* d_running_mean, float* d_running_var, float* d_mean,
                       float* d_var, float* d_scale, float* d_shift, void* d_ws, size_t ws_bytes, void* stream);
int cv_sp_bn_backward_f32(const float* d_x, const float* d_dy, const float* d_y, long long n, int c, int ld,
                          const float* d_mean, const float* d_var, float eps, const float* d_gamma, float* d_dgamma,
                          float* d_dbeta, float* d_dx, float* d_dres, void* d_ws, size_t ws_bytes, void* stream);

/* cv_sp_bn_backward_f32 with a second output for the input-gradient convolution of the layer below (the eval path's hl-format
 * kernels on the transposed map): d_dx_hl = d_dx * s as fp16 pairs, s the power of two that put the PREVIOUS call's largest
 * |dx| of this layer into [2^9, 2^10) - a factor of 64 below the fp16 range; *range_flag is raised beyond it.  d_slot =
 * CV_BN_SLOT_WORDS 32-bit words of the layer that live across steps: [0, 4096) receive this call's largest |dx| per workgroup
 * (bits of non-negative floats, plain stores), [4096, 8192) hold the previous step's (the caller copies the first half there
 * and zeroes it between steps; all zero = unknown: s = 1), [8192] receives 1 / s as a float for cv_conv_desc.acc_scale_dev.
 * c % 32 == 0, ld % 32 == 0, 128-byte aligned rows.  d_dx_hl and d_slot may both be NULL (no twin).  d_relu_bits (optional): the
 * ReLU mask as cv_sp_affine_hl_f32 wrote it, read instead of d_y (which may then be NULL). */
#define CV_BN_SLOT_WORDS 8200
int cv_sp_bn_backward_hl_f32(const float* d_x, const float* d_dy, const float* d_y, long long n, int c, int ld,
                             const float* d_mean, const float* d_var, float eps, const float* d_gamma, float* d_dgamma,
                             float* d_dbeta, float* d_dx, float* d_dres, void* d_ws, size_t ws_bytes, float* d_dx_hl,
                             uint32_t* d_slot, int32_t* range_flag, const uint32_t* d_relu_bits, void* stream);

/* Multi-tensor copy with a device-side guard: h_dst[i][0 .. h_bytes[i]) = h_src[i][...] for i < n (device pointers in host
 * arrays, sizes multiples of 4 bytes; ceil(n / 96) launches) UNLESS *flag != 0 when the launch runs (flag: device-visible
 * int32, NULL = always copy).  The training step snapshots the BatchNorm running statistics with it in front of every
 * forward: once a forward has left the fp16 range (cv_conv_desc.range_flag, sticky until the host resets it) the snapshot stays
 * the state before the FIRST flagged step, whatever was queued since - the host restores from it when it notices
 * (canonicalvoting_amd/train.py; the reference's BatchNorm statistics, train_joint.py:250, see every batch exactly once).
 * Asynchronous. */
int cv_sp_copy_unless_flag(const void* const* h_src, void* const* h_dst, const long long* h_bytes, int n, const int32_t* flag,
                           void* stream);

/* y = relu?(x * scale + shift + residual): MinkowskiBatchNorm (eval) / MinkowskiReLU / the residual add of
 * BasicBlock on feature rows; scale, shift and residual may each be NULL, a shift only together with a scale
 * (CV_EINVAL otherwise: the kernels apply the pair or neither). */
int cv_sp_affine_f32(const float* d_x, long long n, int c, int x_ld, const float* d_scale,
                     const float* d_shift, const float* d_residual, int res_ld, int relu, float* d_y, int y_ld,
                     void* stream);
/* The same pass with a second output: d_y_hl receives the values of d_y in the hl format (the fp16 pairs the hl-format
 * convolutions multiply, cv_conv_desc.in_hl; c % 32 == 0, 128-byte aligned rows) and *range_flag is raised when one exceeds
 * 65000.  The training forward feeds the next convolution from d_y_hl and keeps d_y for autograd (BatchNorm backward, the
 * weight gradient, residual adds).  d_relu_bits (optional, with relu): [n][c / 32] words, bit i of word (r, q) = (y[r][32 q + i] > 0)
 * - what the BatchNorm backward reads instead of the rows of y (cv_sp_bn_backward_hl_f32). */
int cv_sp_affine_hl_f32(const float* d_x, long long n, int c, int x_ld, const float* d_scale, const float* d_shift,
                        const float* d_residual, int res_ld, int relu, float* d_y, int y_ld, float* d_y_hl, int y_hl_ld,
                        uint32_t* d_relu_bits, int32_t* range_flag, void* stream);

/* scale = gamma / sqrt(var + eps), shift = beta - mean * scale (+ bias * scale). */
int cv_sp_bn_fold_f32(const float* d_gamma, const float* d_beta, const float* d_mean, const float* d_var,
                      const float* d_bias, float eps, int c, float* d_scale, float* d_shift, void* stream);

/* Per-point head select of the joint model (eval_joint.py:173-190). */
int cv_head_joint_f32(const float* d_feats, long long n, int ld, int nclasses, int log_scale, float* d_xyz,
                      float* d_scale, float* d_prob, int32_t* d_class, void* stream);

/* 8-channel head of a per-category model (eval_separate.py:170-181): xyz, exp(scale), softmax(obj)[1]. */
int cv_head_separate_f32(const float* d_feats, long long n, int ld, int log_scale, float* d_xyz, float* d_scale,
                         float* d_prob, void* stream);
/* The same head for K models in one launch (the model is blockIdx.y): d_feats[k] is model k's [n][ld] output (host array of
 * K device pointers), the results are [K][n][3], [K][n][3], [K][n] - what K calls of cv_head_separate_f32 write. */
int cv_head_separate_models_f32(const float* const* d_feats, int K, long long n, int ld, int log_scale, float* d_xyz,
                                float* d_scale, float* d_prob, void* stream);

/* ------------------------------------------------------------------------ *
 * One call per scene: eval_joint.py:163-280 (network -> head split -> vote -> decode -> per-class NMS) behind ONE
 * entry point.  Same kernels in the same order as the call-by-call path (cv_sp_scene_plan, cv_net_run_f32,
 * cv_head_joint_f32, cv_hv_forward_f32, cv_decode_f32, cv_nms_obb): bit-identical results.  The host waits twice (level
 * counts of the coordinate plan - the bounds of the points arrive with them - and the decode results); a binding that
 * releases its interpreter lock around foreign calls (ctypes does) keeps it released for the whole scene.
 * ------------------------------------------------------------------------ */
typedef struct cv_scene_desc {
    /* the scene */
    const int32_t* d_coords4;     /* [n][4] (batch, x, y, z), unique rows (eval_joint.py:169).  ONE scene: the spatial row sort does not
                                     sort by the batch column (two launches fewer); rows with different batch indices stay distinct
                                     voxels (every table key carries the index), they only lose their batch-major grouping */
    long long n;
    const float* d_feats;         /* [n][feats_ld] network input features (eval_joint.py:167-168) */
    int feats_ld;
    const float* d_points;        /* [n][3] world points = coords * res (eval_joint.py:193) */
    float res;
    int num_rots;
    /* the network: program of MinkUNet34C.forward (cv_net_run_f32) and the sizes its coordinate plan is built with */
    const cv_net_op* ops; int n_ops;
    const cv_net_buf* bufs; int n_bufs;
    int stem_k, mask_groups;
    long long masked_min_rows;
    int max_channels;             /* widest convolution output (workspace sizing) */
    int use_range_flag;           /* 1: the program runs on fp16 pairs; result.range_flag reports an input beyond the fp16 range */
    float* d_out_feats;           /* [n][out_ld] network output, caller's buffer, caller's row order */
    int out_ld, out_channels;
    int nclasses, log_scale;      /* head split (eval_joint.py:173-190) */
    /* optional: predictions fed to vote + decode instead of the network's (NULL = the network's) */
    const float* d_xyz_in; const float* d_scale_in; const float* d_prob_in; const int32_t* d_class_in;
    int vote_algo;                /* cv_hv_forward_f32 algo (0 auto) */
    cv_decode_params decode;      /* max_iters is taken from max_candidates */
    int max_candidates;           /* capacity of h_cand_idx / h_verdict / h_boxes / h_scores / h_classes / h_pick */
    double nms_threshold;         /* eval_joint.py:273 (0.3) */
    /* scratch: grown by the caller to result.needed_* after a CV_ENOMEM return */
    void* d_ws; size_t ws_bytes;
    float* d_grids; size_t grid_capacity_floats;   /* optional caller buffer for the three grids (6 floats per cell); NULL: in d_ws */
    void* h_pinned; size_t pinned_bytes;           /* >= 256 bytes of page-locked host memory */
    /* host results */
    int64_t* h_cand_idx; int32_t* h_verdict;
    float* h_boxes; float* h_scores; int32_t* h_classes;      /* accepted boxes in acceptance order: [k][8][3], [k], [k] */
    int32_t* h_pick;                                          /* detections after per-class NMS: indices into the box list, class by class */
    int adaptive_split;           /* 1: launch sizing of the coarse-level convolutions by the scenes inside cv_detect_scene_f32 when this
                                     one starts - the one-scene optimum (768 workgroups) below four, 256 from four on (what
                                     bench.py sets by hand for the call-by-call path); 0: the process-wide cv_sp_set_split_target */
    /* optional measurement hook: hipEvent_t handles recorded on `stream` at the scene's start, behind the network, the head
     * split, the vote and the decode (NULL entries are skipped) */
    void* events[5];
    /* launch sizing of THIS call (with masked_min_rows above: the three choices that depend on how many scenes the host keeps
     * in flight - every integer output stays the same bits, the network output moves in fp32 summation order only).  0 = the
     * calling thread's / process-wide value (cv_sp_set_split_target[_thread], cv_hv_set_part_records[_thread]).
     * conv_split_target > 0 overrides adaptive_split. */
    int conv_split_target;        /* workgroups a split coarse-level convolution aims at (library default 768; 256 from four scenes in flight) */
    int vote_part_records;        /* records one workgroup of a hot (tile, plane) takes (library default 4096; 12288 from four in flight) */
    /* 1: vote through cv_hv_forward_peaks_f32 with decode.thresh_high - for a caller that does not read the grids: detections and
     * the raw decode are the same bits, result.d_grid_rot / d_grid_scale hold values only where d_grid_obj >= decode.thresh_high.
     * 0 (a zero-initialised descriptor): full grids, as before. */
    int peak_quotients;
} cv_scene_desc;
typedef struct cv_scene_result {
    int n_cand, n_boxes, n_det, truncated, range_flag, duplicates, out_of_window;
    int scenes_in_flight;          /* scenes inside cv_detect_scene_f32 when this one started (itself included) */
    int dims[3];
    float corner[3];
    long long level_rows[5];
    size_t needed_ws_bytes, needed_grid_floats;
    /* device views into d_ws / d_grids, valid until the next call that uses the same scratch (desc.peak_quotients: rot and scale
     * hold values only at the cells with d_grid_obj >= decode.thresh_high) */
    float* d_grid_obj; float* d_grid_rot; float* d_grid_scale;
    float* d_xyz; float* d_scale; float* d_prob; int32_t* d_class;      /* the network's own head outputs */
    /* host time the call spent (microseconds): [0] coordinate plan incl. its wait for the level counts, [1] enqueueing the network
     * program (~100 launches, no wait), [2] head + vote enqueue, [3] decode incl. its wait for the results + NMS */
    float host_us[4];
} cv_scene_result;
int cv_detect_scene_f32(const cv_scene_desc* desc, cv_scene_result* result, void* stream);

/* ------------------------------------------------------------------------ *
 * B scans in ONE call: cv_detect_scene_f32 over a scene axis.  `scene` describes the batched tensor: d_coords4 [n][4] with the
 * batch column non-decreasing and in [0, num_scenes) (scans collated one after another), d_feats / d_points / d_out_feats and
 * the optional d_*_in predictions over all n rows.  One launch reduces the per-scene row ranges and bounds, ONE coordinate
 * plan and ONE network program run over all rows, one head launch, then ONE vote over the scene axis - every scene on its row
 * range, corner and grid shape, side by side in one launch sequence (cv_hv_forward_scenes_f32, the peaks form under
 * peak_quotients; the vote workspace is the sum of the scenes') - and ONE decode over the same job table
 * (cv_decode_scenes_f32).  The host waits twice
 * per BATCH (level counts - the per-scene ranges and bounds arrive with them - and the decode results); NMS per scene and class
 * on the host.  Scene b is what cv_detect_scene_f32 returns for that scan alone in everything but the network output, which
 * agrees within the network's own tolerance (the batched plan orders and splits the convolutions' sums differently);
 * num_scenes == 1 runs cv_detect_scene_f32's launches and gives its bits (like that call it does not read the batch column).
 * Host result arrays hold num_scenes blocks: scene b's entries at b * max_candidates (h_boxes: b * max_candidates * 24
 * floats), so their capacity is num_scenes * max_candidates.  h_pinned: >= 256 + 64 * num_scenes bytes.  d_grids (optional):
 * the scenes' grid triples one after another, each rounded up to 64 floats - result.needed_grid_floats says how many.
 * CV_EINVAL: num_scenes outside 1..CV_MAX_SCENES and every other bad field before the first device call; after the first
 * wait a scene without rows or a batch column that is not sorted / leaves [0, num_scenes) (the message names the scene).
 * CV_ENOMEM / needed_ws_bytes as cv_detect_scene_f32.
 * ------------------------------------------------------------------------ */
typedef struct cv_scenes_desc {
    cv_scene_desc scene;
    int num_scenes;
} cv_scenes_desc;
typedef struct cv_scenes_result {
    /* per scene */
    int n_cand[CV_MAX_SCENES], n_boxes[CV_MAX_SCENES], n_det[CV_MAX_SCENES], truncated[CV_MAX_SCENES];
    int dims[CV_MAX_SCENES][3];
    float corner[CV_MAX_SCENES][3];
    long long row0[CV_MAX_SCENES], rows[CV_MAX_SCENES];       /* the scene's rows of the batched tensor */
    float* d_grid_obj[CV_MAX_SCENES]; float* d_grid_rot[CV_MAX_SCENES]; float* d_grid_scale[CV_MAX_SCENES];
    /* shared */
    int range_flag, duplicates, out_of_window, scenes_in_flight;
    long long level_rows[5];
    size_t needed_ws_bytes, needed_grid_floats;
    float* d_xyz; float* d_scale; float* d_prob; int32_t* d_class;      /* the network's head outputs over all rows */
    float host_us[4];              /* as cv_scene_result, per batch */
} cv_scenes_result;
int cv_detect_scenes_f32(const cv_scenes_desc* desc, cv_scenes_result* result, void* stream);

/* ------------------------------------------------------------------------ *
 * One call per SEPARATE-mode scene: eval_separate.py:162-264 (K per-category 8-channel models on one scan) behind one entry
 * point: the coordinate plan once, K network programs (cv_net_run_f32, one after another on the stream, sharing the plan and
 * one arena; or batched over a model axis, see models_per_pass), K heads (cv_head_separate_f32), ONE vote over the category axis (cv_hv_forward_cat_f32), ONE decode over it
 * (cv_decode_cat_f32: one host wait) and NMS per category on the host.  Category k is bit for bit the call-by-call path of
 * model k.  1 <= num_models <= CV_MAX_CATEGORIES; every field is validated before the first device call.
 * ------------------------------------------------------------------------ */
typedef struct cv_scene_separate_desc {
    const int32_t* d_coords4; long long n;     /* as cv_scene_desc */
    const float* d_feats; int feats_ld;
    const float* d_points; float res; int num_rots;
    int num_models;                            /* K */
    const cv_net_op* const* ops; const int* n_ops;        /* [K]: program of model k */
    const cv_net_buf* const* bufs; const int* n_bufs;     /* [K] */
    int stem_k, mask_groups;
    long long masked_min_rows;
    int max_channels;                          /* widest convolution output over the K programs */
    int use_range_flag;                        /* 1: the programs run on fp16 pairs; result.range_flag bit k reports model k */
    float* const* d_out_feats;                 /* [K] network outputs [n][out_ld], caller's buffers, caller's row order */
    int out_ld, out_channels;
    int log_scale;                             /* head (eval_separate.py:170-181) */
    /* optional: predictions fed to vote + decode instead of the networks' (NULL = the networks'): [K][n][3], [K][n][3], [K][n] */
    const float* d_xyz_in; const float* d_scale_in; const float* d_prob_in;
    int vote_algo;
    cv_decode_params decode;                   /* max_iters is taken from max_candidates; separate mode: elim_hi_plus1 = 0 */
    int max_candidates;                        /* per category */
    double nms_threshold;                      /* eval_separate.py (0.3) */
    void* d_ws; size_t ws_bytes;               /* grown by the caller to result.needed_ws_bytes after CV_ENOMEM */
    void* h_pinned; size_t pinned_bytes;       /* >= 64 + 64 * K bytes of page-locked host memory */
    /* host results, category k at k * max_candidates entries */
    int64_t* h_cand_idx; int32_t* h_verdict;   /* [K][max_candidates] */
    float* h_boxes; float* h_scores;           /* [K][max_candidates][8][3], [K][max_candidates] */
    int32_t* h_det_cat; int32_t* h_det_box;    /* [K * max_candidates]: detection j = box h_det_box[j] of category h_det_cat[j] */
    void* events[5];                           /* optional: scene start, behind the networks, the heads, the vote, the decode */
    int conv_split_target, vote_part_records;  /* launch sizing of this call (0 = thread / process-wide), as cv_scene_desc */
    /* 0: the K programs one after another on one arena (cv_net_run_f32 K times, K head launches).  G >= 1: passes of up to G
     * models through cv_net_run_models_f32 (the last pass may be shorter, G > K means K) and ONE head launch
     * (cv_head_separate_models_f32): same bits, about K x fewer network launches.  G arenas and G convolution workspaces
     * live at once - result.needed_ws_bytes says how much.  Needs d_model_params.  Negative: CV_EINVAL. */
    int models_per_pass;
    const void* d_model_params;                /* device table [n_ops][K] (cv_net_models_params_fill) of the K programs, or NULL */
} cv_scene_separate_desc;
typedef struct cv_scene_separate_result {
    int n_cand[CV_MAX_CATEGORIES], n_boxes[CV_MAX_CATEGORIES], truncated[CV_MAX_CATEGORIES];
    int n_det, range_flag, duplicates, out_of_window;     /* range_flag: bit k = model k's input beyond the fp16 range */
    int dims[3];
    float corner[3];
    long long level_rows[5];
    size_t needed_ws_bytes;
    /* device views into d_ws, valid until the next call that uses the same scratch: grids [K][X][Y][Z] (+[2], [3]), the networks'
     * head outputs [K][n][3], [K][n][3], [K][n] */
    float* d_grid_obj; float* d_grid_rot; float* d_grid_scale;
    float* d_xyz; float* d_scale; float* d_prob;
    float host_us[4];                          /* plan + wait, network enqueue, heads + vote enqueue, decode + wait + NMS */
} cv_scene_separate_result;
int cv_detect_scene_separate_f32(const cv_scene_separate_desc* desc, cv_scene_separate_result* result, void* stream);

/* ------------------------------------------------------------------------ *
 * A scene from a RAW point cloud in ONE call: voxelise (cv_sp_quantize_f32 / _f64), gather what the scene needs by the
 * first-point index (ONE cv_sp_voxel_rows_f32 launch in joint mode; separate mode: one per 8 gather jobs, 1 + 3 K jobs), then
 * cv_detect_scene_f32 / cv_detect_scene_separate_f32 on the gathered arrays - the same launches as the three pieces issued by
 * the caller, so every output is the same bits.  The descriptor EMBEDS the scene descriptor unchanged behind a raw-cloud front.
 * In `scene`, d_coords4, n, d_feats, feats_ld, d_points and the d_*_in predictions must be NULL / 0 (the call fills a private
 * copy; scene.res is taken from quantization_size), everything else is as for the scene call, with two differences:
 *   - d_out_feats has room for M rows (front.m): the voxel count is not known before the call; result.n rows are written;
 *   - d_ws also holds the front's scratch, carved from its head (quantise workspace, two count words, [m][in_channels]
 *     features, [m][3] points, the gathered predictions; 256-byte aligned carves); the rest is passed on to the scene call.
 *     needed_ws_bytes is the sum of both parts, also after CV_ENOMEM from either; the voxelisation is bit-reproducible, so is
 *     the repeat on a larger workspace.
 * The host waits THREE times: for the voxel count (the row count n is a host argument of every plan kernel; carrying it on the
 * device through them is not done here), the level counts and the decode results.  events[0] is recorded in front of the
 * voxelisation, the other events and host_us are the scene call's.  Rejected points (cv_sp_quantize_*: a non-finite
 * component, a voxel outside the key window): CV_EINVAL, result.rejected holds the count, nothing further is launched.
 * Every field of the front is validated before the first device call.
 * ------------------------------------------------------------------------ */
typedef struct cv_points_front {
    const void* d_raw_points; long long m, points_ld; int points_f64;   /* [m][points_ld] fp32, or fp64 when points_f64 != 0, as cv_sp_quantize_* */
    double quantization_size;                                            /* voxel edge; also the scene's res (as float) */
    const float* d_raw_feats; long long raw_feats_ld; int in_channels;   /* [m][raw_feats_ld], the first in_channels columns are the network's input */
    int recentre_from;                                                   /* cv_gather_job.recentre_from of the features; -1: none */
    /* optional raw-point-aligned predictions fed to vote + decode (NULL = the network's; all or none): [m][3], [m][3], [m], [m];
     * separate mode: [K][m][3], [K][m][3], [K][m] and d_raw_class NULL */
    const float* d_raw_xyz; const float* d_raw_scale; const float* d_raw_prob; const int32_t* d_raw_class;
    /* the voxeliser's outputs, caller's buffers: [m][4] (16-byte aligned, as cv_sp_quantize_* asks), [m], [m] (d_inverse may be
     * NULL); the first result.n rows of d_coords4 / d_index */
    int32_t* d_coords4; int32_t* d_index; int32_t* d_inverse;
} cv_points_front;
typedef struct cv_points_desc { cv_points_front front; cv_scene_desc scene; } cv_points_desc;
typedef struct cv_points_separate_desc { cv_points_front front; cv_scene_separate_desc scene; } cv_points_separate_desc;
typedef struct cv_points_result {
    cv_scene_result scene;             /* needed_ws_bytes: front + scene call */
    long long n;                       /* voxels = rows of the scene */
    int rejected;                      /* cv_sp_quantize_*'s count; != 0: CV_EINVAL */
    float host_us_front;               /* host microseconds of carve + voxelisation (its wait included) + gather enqueue */
    size_t front_ws_bytes;             /* the head of d_ws the front took */
    /* device views into d_ws, valid until the next call on the same scratch: gathered features [n][in_channels], world points
     * [n][3], predictions (NULL when none were given) */
    float* d_feats; float* d_points; float* d_xyz_in; float* d_scale_in; float* d_prob_in; int32_t* d_class_in;
} cv_points_result;
typedef struct cv_points_separate_result {
    cv_scene_separate_result scene;
    long long n; int rejected; float host_us_front; size_t front_ws_bytes;
    float* d_feats; float* d_points; float* d_xyz_in; float* d_scale_in; float* d_prob_in;      /* predictions [K][n][3], [K][n][3], [K][n] */
} cv_points_separate_result;
int cv_detect_points_f32(const cv_points_desc* desc, cv_points_result* result, void* stream);
int cv_detect_points_separate_f32(const cv_points_separate_desc* desc, cv_points_separate_result* result, void* stream);
/* ------------------------------------------------------------------------ *
 * SUN RGB-D proposal sampler on the device (sunrgbd/brnetcanon.py:123-159 behind the 7-argument vote; hv_proposals.hip,
 * DESIGN.md 4.2b).  Both entry points validate every field on the host before their first device call (CV_EINVAL with
 * cv_last_error) and neither waits for the stream.  Built without FMA contraction: every expression is evaluated as written.
 *
 * cv_prop_columns_f32: d_grid_obj [X][Y][Z] (dims = X, Y, Z) -> per (x, z) column c = x * Z + z
 *   m = maximum over y, d_yidx[c] = the FIRST y that attains it; NaN counts as the maximum and the first NaN wins
 *   (torch.max / torch.argmax, numpy); d_dist[c] = (m + 1e-7f) ^ pow: sqrtf for pow == 0.5, else pow in fp64 rounded once.
 *   A second launch of ONE workgroup: d_flags[1] = a non-finite dist was seen, d_flags[0] = uniform taken = that or the sum of
 *   dist (fp64, fixed order) below 1e-7f - every dist is then 1.0f (:128-129); d_cdf[c] = inclusive prefix sum of dist in
 *   fp64, non-decreasing, in an order that depends on X * Z alone: the same bytes on every run and stream.
 *   dims > 0, X * Z <= 2^30, X * Y * Z < 2^31.
 *
 * cv_prop_select_f32: the while loop of :135-159 as ONE workgroup, over a budget of `rounds` rounds of `per_round` draws.
 *   Exactly one of d_draws / d_uniform:
 *     d_draws   int64 [rounds][per_round] flat indices into [X][Z] (an index outside the map is clamped into it);
 *     d_uniform f32 [rounds][per_round] in [0, 1): t = u * d_cdf[last] in fp64, the cell is the first one whose cdf exceeds
 *               t (bisection), the last cell when none does.
 *   Per draw s: ix = s / Z, iz = s % Z, iy = d_yidx[s]; world = (float(i) * res) + corner (two fp32 roundings per component);
 *   scale row = d_grid_scale[ix][iy][iz][:]; d2 = ((dx * dx + dy * dy) + dz * dz) in fp32 against every seed (a NaN wins the
 *   minimum, as in torch.min); near = sqrtf(min d2) < radius.
 *   Per round, in draw order: no draw near -> all per_round draws are kept, else the near ones; kept rows are appended at
 *   start + rows kept so far, rows beyond num_proposal are dropped, and the walk stops as soon as num_proposal rows exist
 *   (later rounds are not evaluated).  Only rows start .. filled - 1 of d_cand / d_scale [num_proposal][3] are written.
 *   d_info = {filled, rounds_used of this call}; with h_info (page-locked) a copy of it is enqueued on the stream.
 *   start > 0 continues a sample that a previous call left short.  d_ws: cv_prop_workspace_bytes of per_round.
 *
 * cv_prop_cloud_ranges_i32: per cloud b of a batched coordinate set d_coords4 [n][4] (batch, x, y, z; batch non-decreasing,
 *   as cv_sp_quantize_* writes it) ONE launch, workgroup b: d_out[b] = {first row, end row, min x, y, z, max x, y, z}
 *   (a cloud without rows: first = end, min = INT32_MAX, max = INT32_MIN); with h_out a copy is enqueued on the stream.
 * ------------------------------------------------------------------------ */
typedef struct cv_prop_select_desc {
    const float* d_grid_scale;                 /* [X][Y][Z][3] */
    const int32_t* d_yidx;                     /* [X * Z] (cv_prop_columns_f32); a value outside [0, Y) is clamped */
    const double* d_cdf;                       /* [X * Z]; read in uniform mode only (may be NULL with d_draws) */
    int dims[3];                               /* X, Y, Z */
    float res; float corner[3];                /* cell edge, grid origin (corners[0]) */
    const float* d_seeds; int n_seeds;         /* vote points [n_seeds][3], n_seeds >= 1 */
    float radius;                              /* 0.3f */
    const int64_t* d_draws; const float* d_uniform;       /* exactly one */
    int rounds, per_round;                     /* >= 1 */
    int num_proposal, start;                   /* P >= 1, 0 <= start <= P */
    float* d_cand; float* d_scale;             /* [P][3] */
    int32_t* d_info; int32_t* h_info;          /* {filled, rounds_used}; h_info may be NULL */
    void* d_ws; size_t ws_bytes;
} cv_prop_select_desc;
size_t cv_prop_workspace_bytes(int per_round);
int cv_prop_columns_f32(const float* d_grid_obj, const int* dims, double pow, float* d_dist, int32_t* d_yidx, double* d_cdf,
                        int32_t* d_flags, void* stream);
int cv_prop_select_f32(const cv_prop_select_desc* desc, void* stream);
int cv_prop_cloud_ranges_i32(const int32_t* d_coords4, long long n, int n_clouds, int32_t* d_out, int32_t* h_out, void* stream);

/* sizeof of the structures above as the LIBRARY was compiled (a binding that mirrors them field by field compares) */
size_t cv_sizeof_prop_select_desc(void);
size_t cv_sizeof_gather_job(void);
size_t cv_sizeof_scan_rows_desc(void);
size_t cv_sizeof_sym_loss_desc(void);
size_t cv_sizeof_row_loss_desc(void);
size_t cv_sizeof_sym_rows_desc(void);
size_t cv_sizeof_points_desc(void);
size_t cv_sizeof_points_separate_desc(void);
size_t cv_sizeof_points_result(void);
size_t cv_sizeof_points_separate_result(void);
size_t cv_sizeof_decode_scene_job(void);
size_t cv_sizeof_scenes_desc(void);
size_t cv_sizeof_scenes_result(void);

#ifdef __cplusplus
}
#endif
#endif /* CV_HIP_H */
