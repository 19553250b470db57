// One C call per scene: eval_joint.py:163-280 behind a single C-ABI entry point.
//
//   coordinate plan (cv_sp_scene_plan) -> MinkUNet34C forward (cv_net_run_f32) -> head split (cv_head_joint_f32)
//   -> vote (cv_hv_forward_f32) -> decode (cv_decode_f32) -> per-class NMS (cv_nms_obb)
//
// The Python pipeline issues the same entry points one by one (~40 ctypes calls, tensor allocations and pointer tables
// per scene, every one of them with the GIL held); a host that keeps several scenes in flight from several threads
// (bench.py: eight) then serialises the enqueue work of all of them.  Here a scene thread makes ONE foreign call - the
// GIL is released for its whole duration - and the host waits twice inside it: for the level counts of the coordinate
// plan (the bounds of the points, reduced in front of the plan, arrive with them: no wait of their own for the vote
// grid's shape) and for the decode results.  Same kernels, same launch order, same arguments: results are bit-identical
// to the call-by-call path (tests/test_scene_call_gpu.py).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cv_common.h"

namespace {

struct Carver {
    char* base; size_t off = 0, cap;
    Carver(void* p, size_t c) : base(static_cast<char*>(p)), cap(c) {}
    // returns nullptr when the workspace is too small; `need` keeps counting so that the caller learns the full size
    template <typename T> T* take(size_t count) {
        off = cv_align_up(off, 256);
        T* r = (base && off + count * sizeof(T) <= cap) ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return r;
    }
};

std::atomic<int> g_scenes_inside{0};
struct SceneCount {
    int before;
    bool set_target, set_records;
    int prev_target = 0, prev_records = 0;
    // the launch sizing of THIS call (cv_scene_desc.conv_split_target / vote_part_records / adaptive_split) lives in the calling
    // thread's values for the duration of the call: two hosts with different policies in one process do not see each other
    SceneCount(bool adaptive, int split_target, int part_records)
        : before(g_scenes_inside.fetch_add(1, std::memory_order_relaxed)), set_target(adaptive || split_target > 0),
          set_records(part_records > 0) {
        // adaptive: scenes in flight (this one included) when the scene starts: the other scenes fill the chip from about four on,
        // below that the deeper splits of the one-scene optimum pay (profiles/r3/split_target_8streams.txt)
        if (set_target) prev_target = cv_sp_set_split_target_thread(split_target > 0 ? split_target : before + 1 >= 4 ? 256 : 768);
        if (set_records) prev_records = cv_hv_set_part_records_thread(part_records);
    }
    ~SceneCount() {
        if (set_target) cv_sp_set_split_target_thread(prev_target);
        if (set_records) cv_hv_set_part_records_thread(prev_records);
        g_scenes_inside.fetch_sub(1, std::memory_order_relaxed);
    }
};

// stage marks (the caller's events, recorded on the stream) and host laps (result.host_us) of one scene call
struct StageClock {
    void* const* events; hipStream_t st; float* host_us;
    std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
    hipError_t mark(int i) const { return events[i] ? hipEventRecord(static_cast<hipEvent_t>(events[i]), st) : hipSuccess; }
    void lap(int i) {
        const auto t = std::chrono::steady_clock::now();
        host_us[i] += std::chrono::duration<float, std::micro>(t - t_prev).count();
        t_prev = t;
    }
};

// The front of a scene call, the same for the joint and the separate mode: bounds of the points, coordinate plan, level
// sizes, vote grid shape, and what the network programs need from them.
struct SceneFront {
    // from either descriptor
    const int32_t* d_coords4; long long n; const float* d_points; float res;
    int stem_k, mask_groups; long long masked_min_rows; int max_channels;
    float* h_minmax;                    // pinned: 6 floats (the landing words of the range flags follow at +64 bytes)
    // carve(): the plan's buffers (cv_sp_scene_plan_layout)
    cv_scene_plan_layout lay;
    void* mm_ws; int32_t* ibuf; unsigned long long* kbuf; char* sort_ws; char* lev_ws;
    // run()
    cv_scene_maps off;
    long long rows[5];
    float mn[3]; int dims[3]; size_t cells;
    const int32_t* maps[CV_NET_MAP_SLOTS]; const int32_t* perms[CV_NET_PERM_SLOTS];
    size_t conv_ws_b;

    template <class D> explicit SceneFront(const D* d)
        : d_coords4(d->d_coords4), n(d->n), d_points(d->d_points), res(d->res), stem_k(d->stem_k), mask_groups(d->mask_groups),
          masked_min_rows(d->masked_min_rows), max_channels(d->max_channels), h_minmax(static_cast<float*>(d->h_pinned)) {}

    // the scene axis (cv_detect_scenes_f32): B > 1 scenes in the batch column; their row ranges and bounds land in the pinned
    // block from +256 bytes on (16 words per scene, cv_hv_scene_bounds_async_ex) and the grid shapes are the caller's to derive.
    // B <= 1: the one scene's front - all rows, bounds in the first six pinned words, the batch column not read
    int num_scenes = 0;
    const int32_t* h_bounds() const { return reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(h_minmax) + 256); }

    // the first five carves of both modes; false when one of them did not fit
    bool carve(Carver& cv) {
        mm_ws = cv.take<char>(cv_hv_minmax_workspace_bytes());
        cv_sp_scene_plan_layout(n, stem_k, mask_groups, masked_min_rows, &lay);
        ibuf = cv.take<int32_t>((size_t)lay.int_words);
        kbuf = cv.take<unsigned long long>((size_t)lay.key_words);
        sort_ws = cv.take<char>(lay.sort_ws_bytes);
        lev_ws = cv.take<char>(lay.levels_ws_bytes);
        return mm_ws && ibuf && kbuf && sort_ws && lev_ws;
    }

    // d_zero_word: a device word that the bounds reduction's final launch zeroes on its way (or NULL)
    template <class R> int run(int32_t* d_zero_word, R* r, StageClock& clock, void* stream) {
        // ---- bounds of the points (the vote grid's origin and shape): reduced first, read after the plan's own host wait
        // (the one-workgroup final launch of the bounds also fills the eight bound words at the head of the sort's workspace)
        int rc = num_scenes > 1
                     ? cv_hv_scene_bounds_async_ex(d_coords4, d_points, n, num_scenes, const_cast<int32_t*>(h_bounds()), mm_ws,
                                                   cv_hv_minmax_workspace_bytes(), d_zero_word, reinterpret_cast<int32_t*>(sort_ws),
                                                   stream)
                     : cv_hv_minmax_async_ex(d_points, n, h_minmax, mm_ws, cv_hv_minmax_workspace_bytes(), d_zero_word,
                                             reinterpret_cast<int32_t*>(sort_ws), stream);
        if (rc != CV_OK) return rc;
        int32_t *c_coords[5], *c_vals[5];
        unsigned long long* c_keys[5];
        for (int i = 0; i < 5; ++i) {
            c_coords[i] = ibuf + lay.coords[i];
            c_keys[i] = kbuf + (size_t)lay.cap * i;
            c_vals[i] = ibuf + lay.vals[i];
        }
        int32_t counts_h[8] = {0};
        rc = cv_sp_scene_plan_ex(d_coords4, n, ibuf + lay.perm, ibuf + lay.inv, c_coords, c_keys, c_vals, lay.cap, ibuf + lay.counts,
                                 counts_h, stem_k, mask_groups, masked_min_rows, ibuf + lay.arena, (size_t)(lay.int_words - lay.arena),
                                 &off, sort_ws, lay.sort_ws_bytes, lev_ws, lay.levels_ws_bytes,
                                 /* one scene: the sort skips its batch digit */ num_scenes <= 1, stream,
                                 /* bound words filled above */ true);
        if (rc != CV_OK) return rc;
        // (the plan waited for an event recorded behind the bounds reduction: the pinned bounds and row ranges are valid)
        rc = check_batch_column();
        if (rc != CV_OK) return rc;
        r->duplicates = counts_h[5];
        r->out_of_window = counts_h[6];
        CV_REQUIRE(counts_h[5] == 0 && counts_h[6] == 0, CV_EINVAL,
                   "duplicate coordinates (%d) or coordinates outside the 16-bit key window (%d)", counts_h[5], counts_h[6]);
        clock.lap(0);
        for (int i = 0; i < 5; ++i) { rows[i] = counts_h[i]; r->level_rows[i] = counts_h[i]; }
        rc = one_grid(r);
        if (rc != CV_OK) return rc;
        // ---- for the network programs: map / order slots (mask orders NULL below masked_min_rows) and the convolution workspace
        int masked[5];
        for (int i = 0; i < 5; ++i) masked[i] = off.mask_perm[i] >= 0;
        conv_ws_b = cv_sp_scene_conv_workspace_bytes(rows, masked, mask_groups, max_channels);
        return cv_sp_scene_plan_slots(&lay, &off, rows, masked_min_rows, ibuf, maps, perms);
    }

    // corner and shape of the one vote grid from the pinned bounds (the scene axis derives B of them itself)
    template <class R> int one_grid(R* r) {
        float mx[3];
        for (int k = 0; k < 3; ++k) { mn[k] = h_minmax[k]; mx[k] = h_minmax[3 + k]; r->corner[k] = mn[k]; }
        const int rc = cv_hv_grid_dims_f32(mn, mx, res, dims);
        if (rc != CV_OK) return rc;
        for (int k = 0; k < 3; ++k) r->dims[k] = dims[k];
        cells = (size_t)dims[0] * dims[1] * dims[2];
        return CV_OK;
    }
    int one_grid(cv_scenes_result*) { return CV_OK; }

    // the scene axis: every scene's rows are one run of the batch column, in scene order, and no scene is empty
    int check_batch_column() const {
        for (int b = 0; num_scenes > 1 && b < num_scenes; ++b) {
            const int32_t* w = h_bounds() + 16 * b;
            const long long first = w[0], end = w[1];
            CV_REQUIRE(w[8] == 0 && first >= 0 && end >= first && end <= n, CV_EINVAL,
                       "scene %d: the batch column is not non-decreasing or leaves [0, %d) (rows %lld..%lld)", b, num_scenes, first,
                       end);
            CV_REQUIRE(end > first, CV_EINVAL, "scene %d has no rows (batch index %d does not occur in the batch column)", b, b);
        }
        return CV_OK;
    }
};

// the part of the workspace that depends on the level sizes is not known yet: ask for the fixed part plus a generous guess
template <class R> int fixed_part_too_small(R* r, size_t fixed_end) {
    r->needed_ws_bytes = fixed_end * 2 + ((size_t)256 << 20);
    cv_set_error("scene workspace too small (needs at least %zu bytes)", r->needed_ws_bytes);
    return CV_ENOMEM;
}

// what cv_detect_scene_f32 and cv_detect_scenes_f32 validate before the first device call
int check_joint_arrays(const cv_scene_desc* d, size_t pinned_min) {
    CV_REQUIRE(d->d_coords4 && d->d_feats && d->d_points && d->n > 0 && d->ops && d->bufs && d->n_ops > 0 && d->n_bufs > 0,
               CV_EINVAL, "bad scene descriptor");
    CV_REQUIRE(d->d_out_feats && d->out_ld >= d->out_channels && d->out_channels > 0, CV_EINVAL, "bad network output buffer");
    CV_REQUIRE(d->h_pinned && d->pinned_bytes >= pinned_min && d->d_ws, CV_EINVAL,
               "pinned scratch (>= %zu bytes) and a device workspace are required", pinned_min);
    CV_REQUIRE(d->h_boxes && d->h_scores && d->h_classes && d->h_cand_idx && d->h_verdict && d->h_pick && d->max_candidates > 0,
               CV_EINVAL, "null result arrays");
    return CV_OK;
}
int check_joint_sizing(const cv_scene_desc* d) {
    CV_REQUIRE(d->conv_split_target >= 0 && d->vote_part_records >= 0, CV_EINVAL, "negative launch sizing");
    CV_REQUIRE(d->vote_algo >= 0 && d->vote_algo <= 2, CV_EINVAL, "vote_algo out of range (%d: 0 auto, 1 direct, 2 tiles)", d->vote_algo);
    return CV_OK;
}

// per-class NMS (eval_joint.py:270-280) of one scene's boxes: kept boxes as indices into the decode's box list, class by class.
// Returns the number of detections, or a negative error.
int nms_per_class(const cv_scene_desc* d, int n_boxes, const float* h_boxes, const float* h_scores, const int32_t* h_classes,
                  int32_t* h_pick) {
    int n_det = 0;
    std::vector<float> bc, sc;
    std::vector<int32_t> idx, pick;
    for (int c = 0; c < d->nclasses; ++c) {
        bc.clear(); sc.clear(); idx.clear();
        for (int i = 0; i < n_boxes; ++i)
            if (h_classes[i] == c) {
                bc.insert(bc.end(), h_boxes + (size_t)i * 24, h_boxes + (size_t)i * 24 + 24);
                sc.push_back(h_scores[i]);
                idx.push_back(i);
            }
        if (idx.empty()) continue;
        pick.assign(idx.size(), 0);
        const int k = cv_nms_obb(bc.data(), sc.data(), (int)idx.size(), d->nms_threshold, pick.data());
        if (k < 0) return k;
        for (int j = 0; j < k; ++j) h_pick[n_det++] = idx[(size_t)pick[j]];
    }
    return n_det;
}

}  // namespace

extern "C" {

int cv_detect_scene_f32(const cv_scene_desc* d, cv_scene_result* r, void* stream) {
    CV_REQUIRE(d && r, CV_EINVAL, "null scene descriptor / result");
    int rc = check_joint_arrays(d, 256);
    if (rc != CV_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long n = d->n;
    std::memset(r, 0, sizeof(*r));
    rc = check_joint_sizing(d);
    if (rc != CV_OK) return rc;
    SceneCount in_flight(d->adaptive_split != 0, d->conv_split_target, d->vote_part_records);
    r->scenes_in_flight = in_flight.before + 1;
    Carver cv(d->d_ws, d->ws_bytes);
    StageClock clock{d->events, st, r->host_us};
    CV_HIP_CHECK(clock.mark(0));

    SceneFront f(d);
    int32_t* h_flag = reinterpret_cast<int32_t*>(static_cast<char*>(d->h_pinned) + 64);      // range flag landing word
    const bool plan_fits = f.carve(cv);
    float* xyz = cv.take<float>((size_t)n * 3);
    float* scale = cv.take<float>((size_t)n * 3);
    float* prob = cv.take<float>((size_t)n);
    int32_t* cls = cv.take<int32_t>((size_t)n);
    int32_t* d_flag = cv.take<int32_t>(64);
    if (!plan_fits || !xyz || !scale || !prob || !cls || !d_flag) return fixed_part_too_small(r, cv.off);
    // (the bounds reduction zeroes the range flag: no fill launch)
    rc = f.run(d_flag, r, clock, stream);
    if (rc != CV_OK) return rc;
    const size_t cells = f.cells;

    // ---- what depends on the level sizes and the grid shape
    const size_t arena_b = cv_net_arena_bytes(d->bufs, d->n_bufs, f.rows, 5);
    const size_t vote_ws_b = cv_hv_forward_workspace_bytes(n, d->num_rots, f.dims, d->vote_algo);
    const size_t dec_ws_b = cv_decode_workspace_bytes(f.dims, n, d->max_candidates);
    char* arena = cv.take<char>(arena_b);
    char* conv_ws = cv.take<char>(f.conv_ws_b);
    char* vote_ws = cv.take<char>(std::max<size_t>(vote_ws_b, 256));
    char* dec_ws = cv.take<char>(dec_ws_b);
    float* grids = d->d_grids ? d->d_grids : cv.take<float>(6 * cells);
    r->needed_ws_bytes = cv.off + 4096;
    r->needed_grid_floats = 6 * cells;
    CV_REQUIRE(arena && conv_ws && vote_ws && dec_ws && grids, CV_ENOMEM, "scene workspace too small (needs %zu bytes)", r->needed_ws_bytes);
    CV_REQUIRE(!d->d_grids || d->grid_capacity_floats >= 6 * cells, CV_ENOMEM, "grid buffer too small (needs %zu floats)", 6 * cells);
    float* g_obj = grids;
    float* g_rot = grids + cells;
    float* g_scale = grids + 3 * cells;
    r->d_grid_obj = g_obj; r->d_grid_rot = g_rot; r->d_grid_scale = g_scale;

    // ---- network forward
    const void* ext_ptr[2] = {d->d_feats, d->d_out_feats};
    const int ext_ld[2] = {d->feats_ld, d->out_ld};
    rc = cv_net_run_ex(d->ops, d->n_ops, d->bufs, d->n_bufs, f.rows, 5, arena, arena_b, ext_ptr, ext_ld, f.maps, CV_NET_MAP_SLOTS,
                       f.perms, CV_NET_PERM_SLOTS, conv_ws, f.conv_ws_b, d->use_range_flag ? d_flag : nullptr, /* plan_maps */ true, stream);
    if (rc != CV_OK) return rc;
    clock.lap(1);
    CV_HIP_CHECK(clock.mark(1));
    rc = cv_head_joint_f32(d->d_out_feats, n, d->out_ld, d->nclasses, d->log_scale, xyz, scale, prob, cls, stream);
    if (rc != CV_OK) return rc;
    if (d->use_range_flag) CV_HIP_CHECK(hipMemcpyAsync(h_flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    r->d_xyz = xyz; r->d_scale = scale; r->d_prob = prob; r->d_class = cls;
    CV_HIP_CHECK(clock.mark(2));

    // ---- vote + decode, on the network's predictions or on the caller's (bench.py --predictions teacher)
    const float* v_xyz = d->d_xyz_in ? d->d_xyz_in : xyz;
    const float* v_scale = d->d_scale_in ? d->d_scale_in : scale;
    const float* v_prob = d->d_prob_in ? d->d_prob_in : prob;
    const int32_t* v_cls = d->d_class_in ? d->d_class_in : cls;
    // (peak_quotients: the decode below is the only reader of rot / scale, and it reads them where g_obj >= thresh_high)
    rc = d->peak_quotients
             ? cv_hv_forward_peaks_f32(d->d_points, v_xyz, v_scale, v_prob, n, d->res, d->num_rots, f.mn, f.dims, g_obj, g_rot, g_scale,
                                       vote_ws, std::max<size_t>(vote_ws_b, 256), d->vote_algo, d->decode.thresh_high, stream)
             : cv_hv_forward_f32(d->d_points, v_xyz, v_scale, v_prob, n, d->res, d->num_rots, f.mn, f.dims, g_obj, g_rot, g_scale, vote_ws,
                                 std::max<size_t>(vote_ws_b, 256), d->vote_algo, stream);
    if (rc != CV_OK) return rc;
    CV_HIP_CHECK(clock.mark(3));
    clock.lap(2);
    cv_decode_params prm = d->decode;
    prm.max_iters = d->max_candidates;
    int n_cand = 0, n_boxes = 0, truncated = 0;
    // (events[4] is recorded behind the decode's last launch, in front of its host wait: a device time)
    const DecodeCall dc{g_obj, g_rot, g_scale, f.dims, f.mn, d->res, d->d_points, v_xyz, v_prob, v_cls, n, &prm, 0, dec_ws, dec_ws_b, &n_cand,
                        d->h_cand_idx, d->h_verdict, &n_boxes, d->h_boxes, d->h_scores, d->h_classes, &truncated, stream, d->events[4]};
    rc = cv_decode_run(dc, 1, true);
    if (rc != CV_OK) return rc;
    r->n_cand = n_cand;
    r->n_boxes = n_boxes;
    r->truncated = truncated;
    // (the decode waited for the stream: the range flag of the network's convolutions has landed)
    r->range_flag = d->use_range_flag ? *h_flag : 0;

    rc = nms_per_class(d, n_boxes, d->h_boxes, d->h_scores, d->h_classes, d->h_pick);
    if (rc < 0) return rc;
    r->n_det = rc;
    clock.lap(3);
    return CV_OK;
}

// B scans in one call: the front, the network and the head over all rows, one vote and one decode over the scene axis.
int cv_detect_scenes_f32(const cv_scenes_desc* sd, cv_scenes_result* r, void* stream) {
    CV_REQUIRE(sd && r, CV_EINVAL, "null scene descriptor / result");
    const cv_scene_desc* d = &sd->scene;
    const int B = sd->num_scenes;
    CV_REQUIRE(B >= 1 && B <= CV_MAX_SCENES, CV_EINVAL, "num_scenes out of range (%d, 1..%d)", B, CV_MAX_SCENES);
    int rc = check_joint_arrays(d, 256 + 64 * (size_t)B);
    if (rc != CV_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long n = d->n;
    const int M = d->max_candidates;
    std::memset(r, 0, sizeof(*r));
    rc = check_joint_sizing(d);
    if (rc != CV_OK) return rc;
    CV_REQUIRE(n < (1ll << 31), CV_EINVAL, "n out of range (%lld)", n);
    SceneCount in_flight(d->adaptive_split != 0, d->conv_split_target, d->vote_part_records);
    r->scenes_in_flight = in_flight.before + 1;
    Carver cv(d->d_ws, d->ws_bytes);
    StageClock clock{d->events, st, r->host_us};
    CV_HIP_CHECK(clock.mark(0));

    SceneFront f(d);
    f.num_scenes = B;
    int32_t* h_flag = reinterpret_cast<int32_t*>(static_cast<char*>(d->h_pinned) + 64);      // range flag landing word
    const bool plan_fits = f.carve(cv);
    float* xyz = cv.take<float>((size_t)n * 3);
    float* scale = cv.take<float>((size_t)n * 3);
    float* prob = cv.take<float>((size_t)n);
    int32_t* cls = cv.take<int32_t>((size_t)n);
    int32_t* d_flag = cv.take<int32_t>(64);
    if (!plan_fits || !xyz || !scale || !prob || !cls || !d_flag) return fixed_part_too_small(r, cv.off);
    rc = f.run(d_flag, r, clock, stream);        // wait 1: level counts, and with them the scenes' row ranges and bounds
    if (rc != CV_OK) return rc;

    // ---- per scene: row range, corner, grid shape
    cv_decode_scene_job jobs[CV_MAX_SCENES];
    size_t cells[CV_MAX_SCENES], grid_floats = 0, dec_ws_b = 0;
    const int32_t* hb = f.h_bounds();
    for (int b = 0; b < B; ++b) {
        // (ranges checked by the front, behind its wait; one scene: all rows, the one-scene call's bounds)
        const int32_t* w = hb + 16 * b;
        const long long first = B > 1 ? w[0] : 0, end = B > 1 ? w[1] : n;
        float mn[3], mx[3];
        std::memcpy(mn, B > 1 ? reinterpret_cast<const float*>(w + 2) : f.h_minmax, sizeof(mn));
        std::memcpy(mx, B > 1 ? reinterpret_cast<const float*>(w + 5) : f.h_minmax + 3, sizeof(mx));
        cv_decode_scene_job& j = jobs[b];
        rc = cv_hv_grid_dims_f32(mn, mx, d->res, j.dims);
        if (rc != CV_OK) return rc;
        for (int k = 0; k < 3; ++k) { j.corner[k] = mn[k]; r->corner[b][k] = mn[k]; r->dims[b][k] = j.dims[k]; }
        j.row0 = first; j.n = end - first;
        r->row0[b] = first; r->rows[b] = end - first;
        cells[b] = (size_t)j.dims[0] * j.dims[1] * j.dims[2];
        grid_floats += cv_align_up(6 * cells[b], 64);
        dec_ws_b += cv_decode_workspace_bytes(j.dims, j.n, M);
    }

    // ---- what depends on the level sizes and the grid shapes: one arena, B vote carves (the scenes' votes run side by side in
    // one launch sequence), B decode carves, B grid triples resident together
    const size_t vote_ws_b = std::max<size_t>(cv_hv_forward_scenes_workspace_bytes(jobs, B, d->num_rots, d->vote_algo), 256);
    const size_t arena_b = cv_net_arena_bytes(d->bufs, d->n_bufs, f.rows, 5);
    char* arena = cv.take<char>(arena_b);
    char* conv_ws = cv.take<char>(f.conv_ws_b);
    char* vote_ws = cv.take<char>(vote_ws_b);
    char* dec_ws = cv.take<char>(dec_ws_b);
    float* grids = d->d_grids ? d->d_grids : cv.take<float>(grid_floats);
    r->needed_ws_bytes = cv.off + 4096;
    r->needed_grid_floats = grid_floats;
    CV_REQUIRE(arena && conv_ws && vote_ws && dec_ws && grids, CV_ENOMEM, "scene workspace too small (needs %zu bytes)", r->needed_ws_bytes);
    CV_REQUIRE(!d->d_grids || d->grid_capacity_floats >= grid_floats, CV_ENOMEM, "grid buffer too small (needs %zu floats)", grid_floats);
    for (int b = 0; b < B; ++b) {
        jobs[b].d_grid_obj = grids;
        jobs[b].d_grid_rot = grids + cells[b];
        jobs[b].d_grid_scale = grids + 3 * cells[b];
        r->d_grid_obj[b] = grids; r->d_grid_rot[b] = grids + cells[b]; r->d_grid_scale[b] = grids + 3 * cells[b];
        grids += cv_align_up(6 * cells[b], 64);
    }

    // ---- network forward and head over all rows
    const void* ext_ptr[2] = {d->d_feats, d->d_out_feats};
    const int ext_ld[2] = {d->feats_ld, d->out_ld};
    rc = cv_net_run_ex(d->ops, d->n_ops, d->bufs, d->n_bufs, f.rows, 5, arena, arena_b, ext_ptr, ext_ld, f.maps, CV_NET_MAP_SLOTS,
                       f.perms, CV_NET_PERM_SLOTS, conv_ws, f.conv_ws_b, d->use_range_flag ? d_flag : nullptr, /* plan_maps */ true, stream);
    if (rc != CV_OK) return rc;
    clock.lap(1);
    CV_HIP_CHECK(clock.mark(1));
    rc = cv_head_joint_f32(d->d_out_feats, n, d->out_ld, d->nclasses, d->log_scale, xyz, scale, prob, cls, stream);
    if (rc != CV_OK) return rc;
    if (d->use_range_flag) CV_HIP_CHECK(hipMemcpyAsync(h_flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    r->d_xyz = xyz; r->d_scale = scale; r->d_prob = prob; r->d_class = cls;
    CV_HIP_CHECK(clock.mark(2));

    // ---- one vote over the scene axis, each scene on its rows, corner and shape; then one decode over the same job table
    const float* v_xyz = d->d_xyz_in ? d->d_xyz_in : xyz;
    const float* v_scale = d->d_scale_in ? d->d_scale_in : scale;
    const float* v_prob = d->d_prob_in ? d->d_prob_in : prob;
    const int32_t* v_cls = d->d_class_in ? d->d_class_in : cls;
    rc = d->peak_quotients
             ? cv_hv_forward_peaks_scenes_f32(jobs, B, d->d_points, v_xyz, v_scale, v_prob, d->res, d->num_rots, vote_ws, vote_ws_b,
                                              d->vote_algo, d->decode.thresh_high, stream)
             : cv_hv_forward_scenes_f32(jobs, B, d->d_points, v_xyz, v_scale, v_prob, d->res, d->num_rots, vote_ws, vote_ws_b,
                                        d->vote_algo, stream);
    if (rc != CV_OK) return rc;
    CV_HIP_CHECK(clock.mark(3));
    clock.lap(2);
    cv_decode_params prm = d->decode;
    prm.max_iters = M;
    const DecodeCall dc{nullptr, nullptr, nullptr, nullptr, nullptr, d->res, d->d_points, v_xyz, v_prob, v_cls, 0, &prm, 0, dec_ws, dec_ws_b,
                        r->n_cand, d->h_cand_idx, d->h_verdict, r->n_boxes, d->h_boxes, d->h_scores, d->h_classes, r->truncated, stream,
                        d->events[4]};
    rc = cv_decode_scenes_run(dc, jobs, B);       // wait 2
    if (rc != CV_OK) return rc;
    r->range_flag = d->use_range_flag ? *h_flag : 0;

    // ---- per scene, per class NMS on the host
    for (int b = 0; b < B; ++b) {
        rc = nms_per_class(d, r->n_boxes[b], d->h_boxes + (size_t)b * M * 24, d->h_scores + (size_t)b * M, d->h_classes + (size_t)b * M,
                           d->h_pick + (size_t)b * M);
        if (rc < 0) return rc;
        r->n_det[b] = rc;
    }
    clock.lap(3);
    return CV_OK;
}

size_t cv_sizeof_scenes_desc(void) { return sizeof(cv_scenes_desc); }
size_t cv_sizeof_scenes_result(void) { return sizeof(cv_scenes_result); }

// eval_separate.py:162-264 as one call: the coordinate plan once, the K programs on it one after another (one shared arena:
// they are ordered on the stream) or, with models_per_pass, as launches over a model axis (cv_net_run_models_f32), K heads into [K][n] arrays, ONE vote and ONE decode over the category axis, NMS per category.
int cv_detect_scene_separate_f32(const cv_scene_separate_desc* d, cv_scene_separate_result* r, void* stream) {
    CV_REQUIRE(d && r, CV_EINVAL, "null scene descriptor / result");
    std::memset(r, 0, sizeof(*r));
    const int K = d->num_models;
    CV_REQUIRE(K >= 1 && K <= CV_MAX_CATEGORIES, CV_EINVAL, "num_models out of range (%d, 1..%d)", K, CV_MAX_CATEGORIES);
    CV_REQUIRE(d->d_coords4 && d->d_feats && d->d_points && d->n > 0 && d->ops && d->n_ops && d->bufs && d->n_bufs && d->d_out_feats,
               CV_EINVAL, "bad scene descriptor");
    for (int k = 0; k < K; ++k)
        CV_REQUIRE(d->ops[k] && d->bufs[k] && d->n_ops[k] > 0 && d->n_bufs[k] > 0 && d->d_out_feats[k], CV_EINVAL,
                   "bad program or output buffer of model %d", k);
    CV_REQUIRE(d->out_ld >= d->out_channels && d->out_channels >= 8, CV_EINVAL, "bad network output buffer");
    CV_REQUIRE(d->h_pinned && d->pinned_bytes >= 64 + 64 * (size_t)K && d->d_ws, CV_EINVAL,
               "pinned scratch (>= 64 + 64 K bytes) and a device workspace are required");
    CV_REQUIRE(d->h_boxes && d->h_scores && d->h_cand_idx && d->h_verdict && d->h_det_cat && d->h_det_box && d->max_candidates > 0,
               CV_EINVAL, "null result arrays");
    CV_REQUIRE(!!d->d_xyz_in == !!d->d_scale_in && !!d->d_xyz_in == !!d->d_prob_in, CV_EINVAL, "predictions: all three or none");
    CV_REQUIRE(d->conv_split_target >= 0 && d->vote_part_records >= 0, CV_EINVAL, "negative launch sizing");
    CV_REQUIRE(d->vote_algo >= 0 && d->vote_algo <= 2, CV_EINVAL, "vote_algo out of range (%d: 0 auto, 1 direct, 2 tiles)", d->vote_algo);
    CV_REQUIRE(d->models_per_pass >= 0, CV_EINVAL, "negative models_per_pass (%d)", d->models_per_pass);
    const int G = std::min(d->models_per_pass, K);          // models per pass of the batched network (0: one after another)
    if (G > 0) {
        CV_REQUIRE(d->d_model_params, CV_EINVAL, "models_per_pass needs d_model_params (cv_net_models_params_fill)");
        for (int k = 1; k < K; ++k)
            CV_REQUIRE(d->n_ops[k] == d->n_ops[0] && d->n_bufs[k] == d->n_bufs[0], CV_EINVAL,
                       "models_per_pass: the program of model %d has another length than model 0's", k);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long n = d->n;
    SceneCount in_flight(false, d->conv_split_target, d->vote_part_records);
    Carver cv(d->d_ws, d->ws_bytes);
    StageClock clock{d->events, st, r->host_us};
    CV_HIP_CHECK(clock.mark(0));

    // ---- bounds + coordinate plan, exactly as cv_detect_scene_f32 (one plan for all K models)
    SceneFront f(d);
    int32_t* h_flags = reinterpret_cast<int32_t*>(static_cast<char*>(d->h_pinned) + 64);     // 16 words per model
    const bool plan_fits = f.carve(cv);
    float* xyz = cv.take<float>((size_t)K * n * 3);
    float* scale = cv.take<float>((size_t)K * n * 3);
    float* prob = cv.take<float>((size_t)K * n);
    int32_t* d_flags = cv.take<int32_t>(16 * (size_t)K);
    if (!plan_fits || !xyz || !scale || !prob || !d_flags) return fixed_part_too_small(r, cv.off);
    if (d->use_range_flag) CV_HIP_CHECK(hipMemsetAsync(d_flags, 0, sizeof(int32_t) * 16 * K, st));
    int rc = f.run(nullptr, r, clock, stream);
    if (rc != CV_OK) return rc;
    const size_t cells = f.cells;

    // ---- what depends on the level sizes and the grid shape: one arena (the largest of the K programs'), K vote / decode carves
    size_t arena_b = 0;
    for (int k = 0; k < K; ++k) arena_b = std::max(arena_b, cv_net_arena_bytes(d->bufs[k], d->n_bufs[k], f.rows, 5));
    const size_t vote_ws_b = cv_hv_forward_cat_workspace_bytes(n, d->num_rots, f.dims, d->vote_algo, K);
    const size_t dec_ws_b = cv_decode_cat_workspace_bytes(f.dims, n, d->max_candidates, K);
    // (batched: G arenas and G convolution workspaces live at once)
    const size_t arena_all = G > 0 ? (size_t)G * arena_b : arena_b;
    const size_t conv_ws_all = G > 0 ? cv_net_models_workspace_bytes(f.conv_ws_b, G) : f.conv_ws_b;
    char* arena = cv.take<char>(arena_all);
    char* conv_ws = cv.take<char>(conv_ws_all);
    char* vote_ws = cv.take<char>(std::max<size_t>(vote_ws_b, 256));
    char* dec_ws = cv.take<char>(dec_ws_b);
    float* grids = cv.take<float>(6 * cells * (size_t)K);
    r->needed_ws_bytes = cv.off + 4096;
    CV_REQUIRE(arena && conv_ws && vote_ws && dec_ws && grids, CV_ENOMEM, "scene workspace too small (needs %zu bytes)", r->needed_ws_bytes);
    float* g_obj = grids;
    float* g_rot = grids + cells * K;
    float* g_scale = grids + 3 * cells * K;
    r->d_grid_obj = g_obj; r->d_grid_rot = g_rot; r->d_grid_scale = g_scale;

    // ---- K network programs on the shared plan: in passes of up to G over the model axis, or one after another
    for (int m0 = 0; G > 0 && m0 < K; m0 += G) {
        const int g = std::min(G, K - m0);
        const void* ext_ptr[CV_MAX_CATEGORIES][2];
        const void* const* ext_tab[CV_MAX_CATEGORIES];
        for (int m = 0; m < g; ++m) {
            ext_ptr[m][0] = d->d_feats, ext_ptr[m][1] = d->d_out_feats[m0 + m];
            ext_tab[m] = ext_ptr[m];
        }
        const int ext_ld[2] = {d->feats_ld, d->out_ld};
        rc = cv_net_run_models_ex(d->ops + m0, d->bufs + m0, d->n_ops[0], d->n_bufs[0], g, f.rows, 5, arena, arena_all, ext_tab, ext_ld,
                                  f.maps, CV_NET_MAP_SLOTS, f.perms, CV_NET_PERM_SLOTS, conv_ws, conv_ws_all,
                                  d->use_range_flag ? d_flags + 16 * m0 : nullptr,
                                  static_cast<const cv_net_model_params*>(d->d_model_params) + m0, K, /* plan_maps */ true, stream);
        if (rc != CV_OK) return rc;
    }
    for (int k = 0; G == 0 && k < K; ++k) {
        const void* ext_ptr[2] = {d->d_feats, d->d_out_feats[k]};
        const int ext_ld[2] = {d->feats_ld, d->out_ld};
        rc = cv_net_run_ex(d->ops[k], d->n_ops[k], d->bufs[k], d->n_bufs[k], f.rows, 5, arena, arena_b, ext_ptr, ext_ld, f.maps,
                           CV_NET_MAP_SLOTS, f.perms, CV_NET_PERM_SLOTS, conv_ws, f.conv_ws_b,
                           d->use_range_flag ? d_flags + 16 * k : nullptr, /* plan_maps */ true, stream);
        if (rc != CV_OK) return rc;
    }
    clock.lap(1);
    CV_HIP_CHECK(clock.mark(1));
    if (G > 0) {        // one head launch over the model axis
        rc = cv_head_separate_models_f32(d->d_out_feats, K, n, d->out_ld, d->log_scale, xyz, scale, prob, stream);
        if (rc != CV_OK) return rc;
    }
    for (int k = 0; G == 0 && k < K; ++k) {
        rc = cv_head_separate_f32(d->d_out_feats[k], n, d->out_ld, d->log_scale, xyz + (size_t)k * n * 3, scale + (size_t)k * n * 3,
                                  prob + (size_t)k * n, stream);
        if (rc != CV_OK) return rc;
    }
    if (d->use_range_flag) CV_HIP_CHECK(hipMemcpyAsync(h_flags, d_flags, sizeof(int32_t) * 16 * K, hipMemcpyDeviceToHost, st));
    r->d_xyz = xyz; r->d_scale = scale; r->d_prob = prob;
    CV_HIP_CHECK(clock.mark(2));

    // ---- one vote and one decode over the category axis
    const float* v_xyz = d->d_xyz_in ? d->d_xyz_in : xyz;
    const float* v_scale = d->d_xyz_in ? d->d_scale_in : scale;
    const float* v_prob = d->d_xyz_in ? d->d_prob_in : prob;
    rc = cv_hv_forward_cat_f32(d->d_points, v_xyz, v_scale, v_prob, n, d->res, d->num_rots, f.mn, f.dims, K, g_obj, g_rot, g_scale, vote_ws,
                               std::max<size_t>(vote_ws_b, 256), d->vote_algo, stream);
    if (rc != CV_OK) return rc;
    CV_HIP_CHECK(clock.mark(3));
    clock.lap(2);
    cv_decode_params prm = d->decode;
    prm.max_iters = d->max_candidates;
    const int M = d->max_candidates;
    std::vector<int32_t> classes((size_t)K * M);
    const DecodeCall dc{g_obj, g_rot, g_scale, f.dims, f.mn, d->res, d->d_points, v_xyz, v_prob, nullptr, n, &prm, 0, dec_ws, dec_ws_b,
                        r->n_cand, d->h_cand_idx, d->h_verdict, r->n_boxes, d->h_boxes, d->h_scores, classes.data(), r->truncated, stream,
                        d->events[4]};
    rc = cv_decode_run(dc, K, false);
    if (rc != CV_OK) return rc;
    // (the decode waited for the stream: the range flags of the K programs have landed)
    if (d->use_range_flag)
        for (int k = 0; k < K; ++k) r->range_flag |= h_flags[16 * k] ? (1 << k) : 0;

    // ---- NMS per category (eval_separate.py): detections in category order, highest score first within a category
    int n_det = 0;
    std::vector<int32_t> pick((size_t)M);
    for (int k = 0; k < K; ++k) {
        const int nb = r->n_boxes[k];
        if (nb == 0) continue;
        const int kept = cv_nms_obb(d->h_boxes + (size_t)k * M * 24, d->h_scores + (size_t)k * M, nb, d->nms_threshold, pick.data());
        if (kept < 0) return kept;
        for (int j = 0; j < kept; ++j) { d->h_det_cat[n_det] = k; d->h_det_box[n_det] = pick[(size_t)j]; ++n_det; }
    }
    r->n_det = n_det;
    clock.lap(3);
    return CV_OK;
}

}  // extern "C"

// ---- a scene from a RAW cloud: voxelise -> gather -> the scene call above, as ONE call ------------------------------------
// A front in front of cv_detect_scene_f32 / cv_detect_scene_separate_f32 (their bodies are untouched): its scratch is carved
// from the head of the scene's workspace, the voxeliser's host wait gives the row count, one gather launch (one per eight jobs
// in separate mode) makes the voxel-aligned features, world points and predictions, and the scene call runs on a private copy
// of the descriptor that points at them, with the rest of the workspace.  A third host wait (the voxel count): the plan
// kernels take the row count from the host, carrying it on the device through all of them is not done here.
namespace {

int check_points_front(const cv_points_front& f, bool joint) {
    CV_REQUIRE(f.d_raw_points && f.d_raw_feats && f.d_coords4 && f.d_index, CV_EINVAL, "raw cloud: null pointer argument");
    CV_REQUIRE(f.m > 0 && f.m <= (1ll << 29), CV_EINVAL, "raw cloud: bad point count %lld", f.m);
    CV_REQUIRE(f.points_ld >= 3, CV_EINVAL, "raw cloud: bad row stride %lld", f.points_ld);
    // (as float too: the scene's res and the fp32 voxeliser's divisor)
    CV_REQUIRE(f.quantization_size > 0 && f.quantization_size <= 3.0e38 && (float)f.quantization_size > 0.0f, CV_EINVAL,
               "raw cloud: quantization_size must be positive and finite (got %g)", f.quantization_size);
    CV_REQUIRE(f.in_channels > 0 && f.in_channels <= f.raw_feats_ld, CV_EINVAL, "raw cloud: bad feature width %d (row stride %lld)",
               f.in_channels, f.raw_feats_ld);
    CV_REQUIRE(f.recentre_from <= f.in_channels, CV_EINVAL, "raw cloud: recentre_from %d beyond the feature width %d", f.recentre_from,
               f.in_channels);
    const int given = !!f.d_raw_xyz + !!f.d_raw_scale + !!f.d_raw_prob + (joint ? !!f.d_raw_class : 0);
    CV_REQUIRE(given == 0 || given == (joint ? 4 : 3), CV_EINVAL, "raw cloud: predictions: all %d arrays or none", joint ? 4 : 3);
    CV_REQUIRE(joint || !f.d_raw_class, CV_EINVAL, "raw cloud: separate mode takes no class array");
    return CV_OK;
}

// K: prediction sets ([K][m][..] raw, [K][n][..] gathered); d_class_view: where joint mode's gathered class array is handed
// over (NULL: separate mode, no class array)
template <class PD, class PR, class Inner>
int detect_points(const PD* pd, PR* r, int K, int32_t** d_class_view, Inner inner, void* stream) {
    const bool joint = d_class_view != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    const cv_points_front& f = pd->front;
    auto sd = pd->scene;                            // the private copy the scene call runs on
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long m = f.m;
    const int C = f.in_channels;
    const bool pred = f.d_raw_xyz != nullptr;
    const float res = (float)f.quantization_size;

    // ---- 1. the front's scratch, from the head of the scene's workspace
    Carver cv(sd.d_ws, sd.ws_bytes);
    const size_t q_ws_b = cv_sp_quantize_workspace_bytes(m);
    char* q_ws = cv.take<char>(q_ws_b);
    int32_t* d_counts = cv.take<int32_t>(2);
    float* feats = cv.take<float>((size_t)m * C);
    float* points = cv.take<float>((size_t)m * 3);
    float* xyz = pred ? cv.take<float>((size_t)K * m * 3) : nullptr;
    float* scale = pred ? cv.take<float>((size_t)K * m * 3) : nullptr;
    float* prob = pred ? cv.take<float>((size_t)K * m) : nullptr;
    int32_t* cls = pred && joint ? cv.take<int32_t>((size_t)m) : nullptr;
    const size_t front = cv_align_up(cv.off, 256);
    r->front_ws_bytes = front;
    sd.events[0] = nullptr;                         // (recorded here, in front of the voxelisation)
    const bool fits = front <= sd.ws_bytes && q_ws && d_counts && feats && points && (!pred || (xyz && scale && prob)) &&
                      (!(pred && joint) || cls);
    if (!fits) {
        // the scene call's own size when every point is a voxel, asked with no room at all: it returns from its fixed-part check,
        // in front of its first launch (the pointers are placeholders, never read)
        sd.d_coords4 = f.d_coords4; sd.n = m;
        sd.d_feats = static_cast<const float*>(sd.d_ws); sd.feats_ld = C;
        sd.d_points = static_cast<const float*>(sd.d_ws); sd.res = res;
        sd.ws_bytes = 0;
        const int rc = inner(&sd, &r->scene, stream);
        if (rc != CV_ENOMEM) return rc;
        r->scene.needed_ws_bytes += front;
        cv_set_error("scene workspace too small (needs at least %zu bytes)", r->scene.needed_ws_bytes);
        return CV_ENOMEM;
    }

    // ---- 2. voxelise: the host waits for the voxel count and the rejected count
    if (pd->scene.events[0]) CV_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(pd->scene.events[0]), st));
    int32_t h_counts[2] = {0, 0};
    int rc = f.points_f64
                 ? cv_sp_quantize_f64(static_cast<const double*>(f.d_raw_points), m, f.points_ld, f.quantization_size, 0, nullptr, 0,
                                      f.d_coords4, f.d_index, f.d_inverse, d_counts, h_counts, q_ws, q_ws_b, stream)
                 : cv_sp_quantize_f32(static_cast<const float*>(f.d_raw_points), m, f.points_ld, res, 0, nullptr, 0, f.d_coords4,
                                      f.d_index, f.d_inverse, d_counts, h_counts, q_ws, q_ws_b, stream);
    if (rc != CV_OK) return rc;
    const long long n = h_counts[0];
    r->n = n;
    r->rejected = h_counts[1];
    CV_REQUIRE(h_counts[1] == 0, CV_EINVAL,
               "%d points rejected (a non-finite component, or a voxel outside the supported window: spatial coordinates in "
               "[-32704, 32703])", h_counts[1]);
    CV_REQUIRE(n > 0 && n <= m, CV_EINVAL, "the voxeliser returned %lld voxels of %lld points", n, m);

    // ---- 3. gather: features, world points and predictions of the voxels' first points
    std::vector<cv_gather_job> jobs;
    jobs.push_back({f.d_raw_feats, f.raw_feats_ld, feats, C, C, f.recentre_from});
    for (int k = 0; pred && k < K; ++k) {
        jobs.push_back({f.d_raw_xyz + (size_t)k * m * 3, 3, xyz + (size_t)k * n * 3, 3, 3, -1});
        jobs.push_back({f.d_raw_scale + (size_t)k * m * 3, 3, scale + (size_t)k * n * 3, 3, 3, -1});
        jobs.push_back({f.d_raw_prob + (size_t)k * m, 1, prob + (size_t)k * n, 1, 1, -1});
    }
    if (pred && joint) jobs.push_back({f.d_raw_class, 1, cls, 1, 1, -1});
    for (size_t j0 = 0; j0 < jobs.size(); j0 += CV_GATHER_MAX_JOBS) {
        rc = cv_sp_voxel_rows_f32(f.d_coords4, f.d_index, n, res, j0 == 0 ? points : nullptr, jobs.data() + j0,
                                  (int)std::min<size_t>(CV_GATHER_MAX_JOBS, jobs.size() - j0), stream);
        if (rc != CV_OK) return rc;
    }
    r->d_feats = feats; r->d_points = points; r->d_xyz_in = xyz; r->d_scale_in = scale; r->d_prob_in = prob;
    if (joint) *d_class_view = cls;

    // ---- 4. the scene call on the gathered arrays and the rest of the workspace
    sd.d_coords4 = f.d_coords4; sd.n = n;
    sd.d_feats = feats; sd.feats_ld = C;
    sd.d_points = points; sd.res = res;
    sd.d_xyz_in = xyz; sd.d_scale_in = scale; sd.d_prob_in = prob;
    sd.d_ws = static_cast<char*>(sd.d_ws) + front;
    sd.ws_bytes -= front;
    r->host_us_front = std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - t0).count();
    rc = inner(&sd, &r->scene, stream);
    if (r->scene.needed_ws_bytes) r->scene.needed_ws_bytes += front;
    if (rc == CV_ENOMEM) cv_set_error("scene workspace too small (needs %zu bytes)", r->scene.needed_ws_bytes);
    return rc;
}

}  // namespace

extern "C" {

int cv_detect_points_f32(const cv_points_desc* d, cv_points_result* r, void* stream) {
    CV_REQUIRE(d && r, CV_EINVAL, "null raw-cloud descriptor / result");
    std::memset(r, 0, sizeof(*r));
    int rc = check_points_front(d->front, true);
    if (rc != CV_OK) return rc;
    const cv_scene_desc& s = d->scene;
    CV_REQUIRE(!s.d_coords4 && s.n == 0 && !s.d_feats && s.feats_ld == 0 && !s.d_points && !s.d_xyz_in && !s.d_scale_in && !s.d_prob_in &&
                   !s.d_class_in, CV_EINVAL, "raw cloud: the scene's d_coords4 / n / d_feats / feats_ld / d_points / d_*_in must be NULL / 0");
    CV_REQUIRE(s.ops && s.bufs && s.n_ops > 0 && s.n_bufs > 0 && s.d_out_feats && s.d_ws && s.h_pinned && s.max_candidates > 0, CV_EINVAL,
               "bad scene descriptor");
    CV_REQUIRE(s.vote_algo >= 0 && s.vote_algo <= 2, CV_EINVAL, "vote_algo out of range (%d: 0 auto, 1 direct, 2 tiles)", s.vote_algo);
    // (the class array is joint mode's alone: the shared front hands its carve over through the result)
    auto inner = [r](cv_scene_desc* sd, cv_scene_result* sr, void* st) {
        sd->d_class_in = r->d_class_in;
        return cv_detect_scene_f32(sd, sr, st);
    };
    return detect_points(d, r, 1, &r->d_class_in, inner, stream);
}

int cv_detect_points_separate_f32(const cv_points_separate_desc* d, cv_points_separate_result* r, void* stream) {
    CV_REQUIRE(d && r, CV_EINVAL, "null raw-cloud descriptor / result");
    std::memset(r, 0, sizeof(*r));
    int rc = check_points_front(d->front, false);
    if (rc != CV_OK) return rc;
    const cv_scene_separate_desc& s = d->scene;
    CV_REQUIRE(!s.d_coords4 && s.n == 0 && !s.d_feats && s.feats_ld == 0 && !s.d_points && !s.d_xyz_in && !s.d_scale_in && !s.d_prob_in,
               CV_EINVAL, "raw cloud: the scene's d_coords4 / n / d_feats / feats_ld / d_points / d_*_in must be NULL / 0");
    CV_REQUIRE(s.num_models >= 1 && s.num_models <= CV_MAX_CATEGORIES, CV_EINVAL, "num_models out of range (%d, 1..%d)", s.num_models,
               CV_MAX_CATEGORIES);
    CV_REQUIRE(s.ops && s.n_ops && s.bufs && s.n_bufs && s.d_out_feats && s.d_ws && s.h_pinned && s.max_candidates > 0, CV_EINVAL,
               "bad scene descriptor");
    CV_REQUIRE(s.vote_algo >= 0 && s.vote_algo <= 2, CV_EINVAL, "vote_algo out of range (%d: 0 auto, 1 direct, 2 tiles)", s.vote_algo);
    auto inner = [](cv_scene_separate_desc* sd, cv_scene_separate_result* sr, void* st) {
        return cv_detect_scene_separate_f32(sd, sr, st);
    };
    return detect_points(d, r, s.num_models, nullptr, inner, stream);
}

size_t cv_sizeof_points_desc(void) { return sizeof(cv_points_desc); }
size_t cv_sizeof_points_separate_desc(void) { return sizeof(cv_points_separate_desc); }
size_t cv_sizeof_points_result(void) { return sizeof(cv_points_result); }
size_t cv_sizeof_points_separate_result(void) { return sizeof(cv_points_separate_result); }

}  // extern "C"
