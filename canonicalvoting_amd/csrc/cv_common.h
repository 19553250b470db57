// Shared host-side helpers for libcvhip.so (error reporting, launch checks).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "cv_hip.h"

void cv_set_error(const char* fmt, ...);

#define CV_HIP_CHECK(expr)                                                                  \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            cv_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,   \
                         __LINE__);                                                         \
            return CV_EHIP;                                                                 \
        }                                                                                   \
    } while (0)

#define CV_LAUNCH_CHECK() CV_HIP_CHECK(hipGetLastError())

#define CV_REQUIRE(cond, code, ...)     \
    do {                                \
        if (!(cond)) {                  \
            cv_set_error(__VA_ARGS__);  \
            return (code);              \
        }                               \
    } while (0)

__host__ __device__ static inline size_t cv_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Carves typed sub-buffers out of a caller-provided device workspace.
struct CvCarver {
    char* base;
    size_t off = 0;
    explicit CvCarver(void* p) : base(static_cast<char*>(p)) {}
    template <typename T>
    T* take(size_t count) {
        off = cv_align_up(off, 256);
        T* r = reinterpret_cast<T*>(base + off);
        off += count * sizeof(T);
        return r;
    }
};

// ---- internal batch launches (one launch for the jobs of a whole scene instead of one per map; used by the coordinate
//      plan, cv_sp_scene_plan_ex and cv_sp_scene_maps in net_exec.cpp; C++ linkage, not part of the C ABI) ---------------
struct CvMapJob {            // kernel map: out set looked up in an input set's hash table
    const int32_t* out_coords; long long n_out;
    const unsigned long long* keys; const int32_t* vals; long long cap;
    int k, ts;
    int32_t* nbr;
    const int32_t* compose;  // optional: store compose[row] instead of row (a permutation folded into the map)
    const unsigned* bitmap;  // optional (ts == 1 maps of the set the bitmap was built from): occupancy bits in front of the
    const int32_t* bbox;     // hash probes, see CV_BITMAP_WORDS; bbox = the 8 ints of cv_sp_sort_rows' bounds
    int up;                  // 1: transposed k2s2 map instead - out_coords are the FINE rows (tensor stride ts), keys / vals the
                             // table of the next coarser level, nbr[n_out][8] = parent row in the octant column, -1 elsewhere
    int32_t* nbr3;           // optional (k == 5, ts == 1): the 3x3x3 map of the same set [n_out][27] (rows NOT composed) is built
                             // by the same job - with a trusted bitmap one lane reads a whole (dx, dy) line of five z-bits
    int32_t* mask_words;     // optional (where a 3x3x3 map is built: nbr3, or k == 3): [n_out] bit j = entry j of the row's
                             // 3x3x3 map >= 0 (what the mask orders sort by, CvPermJob.mask_words)
};
constexpr int CV_MAX_MAP_JOBS = 12;
int cv_sp_kernel_maps_batch(const CvMapJob* jobs, int n_jobs, void* stream);
// Occupancy bitmap of a coordinate set over its bounding box (d_bbox: mm[0..2] = min, mm[3..5] = -max per axis, mm[6] =
// -max batch, as left by cv_sp_sort_rows at the start of its workspace; mm[7] = 1 while the bitmap may be trusted): 87 % of a
// scene's kernel-map lookups are misses, each ~2 random probes into a 2 MB table; a bit test against ~0.5 MB with
// neighbouring lookups in the same words answers them.  d_bits: CV_BITMAP_WORDS words, zeroed by the first launch of
// cv_sp_build_levels_zero and filled by its insert pass (insert_all) on the way.  When the box does not fit (or a batch index
// is negative: insert_all then clears mm[7]) the kernels that take the bitmap ignore it (they re-derive the same test from
// the bounds).
constexpr long long CV_BITMAP_WORDS = 1ll << 20;

// cv_sp_build_levels with an extra range of words zeroed by its first launch (d_zero / n_zero, may be null / 0: saves the
// caller's fill launches) and, with d_bbox / d_bits (both or neither; d_bits lies inside the zeroed range), the occupancy bitmap
int cv_sp_build_levels_zero(int32_t* const* d_coords, unsigned long long* const* d_keys, int32_t* const* d_vals,
                            long long n, long long cap, int num_levels, int32_t* d_counts, int32_t* h_counts, void* d_ws,
                            size_t ws_bytes, int32_t* d_zero, long long n_zero, int32_t* d_bbox, uint32_t* d_bits,
                            void* stream);                                                  // sparse_coords.hip

struct CvPermJob {
    const int32_t* nbr; long long n; int K, groups; int32_t* perm; int with_map;
    const int32_t* mask_words;   // optional (K <= 32): bit j of word [row] = nbr[row][j] >= 0, from the map builder (CvMapJob)
};
constexpr int CV_MAX_PERM_JOBS = 8;
int cv_hv_minmax_async_ex(const float* d_points, int64_t n, float* h_minmax6, void* d_ws, size_t ws_bytes, int32_t* d_zero_word,
                          int32_t* d_fill7f, void* stream);                                // hv_vote.hip
// One decode call (hv_decode.hip): what cv_decode_f32 / cv_decode_cat_f32 take, in their order, plus an optional event
// (hipEvent_t) recorded behind the LAST launch, in front of the host's wait for the results - the scene call's "decode done"
// mark is then a device time.  With K categories the grids, predictions, workspace and host outputs hold K blocks.
struct DecodeCall {
    float* d_grid_obj; const float* d_grid_rot; const float* d_grid_scale;
    const int* dims; const float* h_corner3; float res;
    const float* d_points; const float* d_xyz; const float* d_prob; const int32_t* d_class; int64_t n;
    const cv_decode_params* params; int mutate_grid;
    void* d_ws; size_t ws_bytes;
    int* h_n_cand; int64_t* h_cand_idx; int32_t* h_verdict; int* h_n_boxes; float* h_boxes; float* h_scores; int32_t* h_classes;
    int* h_truncated;        // may be NULL
    void* stream; void* ev_done;
};
// need_class: d_class must not be NULL (the joint model's class vote; the separate models pass none: class 0)
int cv_decode_run(const DecodeCall& c, int num_cats, bool need_class);
// The scene axis: the jobs carry grids, dims, corner and row range (c's own are not read); c.d_points / d_xyz / d_prob / d_class
// are the shared arrays, c.d_ws the B carves in job order.  Scene b's host outputs at b, b * max_iters, b * max_iters * 24.
int cv_decode_scenes_run(const DecodeCall& c, const cv_decode_scene_job* jobs, int num_scenes);
// Row ranges and bounds of the B scenes of a batched coordinate set, ONE launch and one copy into pinned memory, no host wait.
// h_out (PINNED, 16 words per scene, valid once the stream's work up to here is done): [0] first row, [1] end row, [2..7] fp32
// min xyz / max xyz of d_points over those rows (the values cv_hv_minmax_async_ex lands for the scene alone), [8] != 0 when a
// row of the range carries another batch index or the ranges do not tile [0, n).  d_ws: cv_hv_minmax_workspace_bytes().
// d_zero_word / d_fill7f: as cv_hv_minmax_async_ex.
int cv_hv_scene_bounds_async_ex(const int32_t* d_coords4, const float* d_points, int64_t n, int num_scenes, int32_t* h_out,
                                void* d_ws, size_t ws_bytes, int32_t* d_zero_word, int32_t* d_fill7f, void* stream);   // hv_vote.hip
int cv_sp_sort_rows_ex(const int32_t* d_coords, long long n, int32_t* d_sorted, int32_t* d_perm, int32_t* d_inv, void* d_ws,
                       size_t ws_bytes, bool single_batch, void* stream, bool bounds_prefilled);           // sparse_coords.hip
int cv_sp_scene_plan_ex(const int32_t* d_input, long long n, int32_t* d_perm, int32_t* d_inv, int32_t* const* d_coords,
                        unsigned long long* const* d_keys, int32_t* const* d_vals, long long cap, int32_t* d_counts,
                        int32_t* h_counts, int stem_k, int mask_groups, long long masked_min_rows,
                        int32_t* d_arena, size_t arena_words, cv_scene_maps* offsets, void* d_sort_ws, size_t sort_ws_bytes,
                        void* d_levels_ws, size_t levels_ws_bytes, bool single_batch, void* stream,
                        bool bounds_prefilled);                                               // net_exec.cpp
// cv_net_run_f32 / cv_net_run_models_f32 for a caller that KNOWS where its maps come from (the scene calls).  plan_maps: the maps
// are the scene plan's, so a validity word per row lies behind every 3x3x3 map with mask orders; the mask-sorted convolutions
// get it as cv_conv_desc.valid_words (the C ABI entry points pass false: their caller's maps may be any)
int cv_net_run_ex(const cv_net_op* ops, int n_ops, const cv_net_buf* bufs, int n_bufs, const long long* level_rows,
                  int n_levels, void* d_arena, size_t arena_bytes, const void* const* ext_ptr, const int* ext_ld,
                  const int32_t* const* maps, int n_maps, const int32_t* const* perms, int n_perms,
                  void* d_ws, size_t ws_bytes, int32_t* range_flag, bool plan_maps, void* stream);           // net_exec.cpp
int cv_net_run_models_ex(const cv_net_op* const* ops, const cv_net_buf* const* bufs, int n_ops, int n_bufs, int K,
                         const long long* level_rows, int n_levels, void* d_arena, size_t arena_bytes,
                         const void* const* const* ext_ptr, const int* ext_ld, const int32_t* const* maps, int n_maps,
                         const int32_t* const* perms, int n_perms, void* d_ws, size_t ws_bytes, int32_t* range_flag,
                         const void* d_params, int params_ld, bool plan_maps, void* stream);                  // net_exec.cpp
// d_ws: (sum of groups) * 2048 ints, zero-filled by the call unless pre_zeroed
int cv_sp_mask_perms_batch(const CvPermJob* jobs, int n_jobs, void* d_ws, size_t ws_bytes, void* stream,
                           bool pre_zeroed);                                                // conv_prep.hip

// cv_sp_conv_f32 over the model axis (cv_net_run_models_f32): `d` describes model 0; the operands of model m are model 0's
// plus m x the byte strides (0 = shared), its packed weights / affine / acc_scale row m of d_params, its workspace
// d->ws + m x ws_stride (d->ws_bytes is ONE model's share), its range flag d->range_flag + 16 m.  out_ext: the output is the
// caller's tensor ext_out[m].  fp16-pair hl programs only (and their matrix-core stem); CV_EINVAL otherwise.
struct CvConvModels {
    int models;
    const cv_net_model_params* d_params;
    long long in_stride, in2_stride, res_stride, out_stride, ws_stride;
    int out_ext;
    float* ext_out[CV_MAX_CATEGORIES];
};
int cv_sp_conv_models_f32(const cv_conv_desc* d, const CvConvModels* mm, void* stream);          // sparse_conv.hip
