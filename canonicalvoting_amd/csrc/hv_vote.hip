// Canonical vote accumulation for gfx950 (MI355X).
//
// Replaces houghvoting/src/hv_cuda_kernel.cu (forward :12-97, average :100-119,
// backward :168-261, host shape logic :121-165) behind the C ABI of include/cv_hip.h.
//
// Compiled with -ffp-contract=off: the per-vote geometry (offset, grid position,
// bounds test, floor, trilinear weights) is the strict fp32 operation sequence of
// the reference source, so cell indices and per-vote contributions are bit-identical
// to oracle/hv_oracle.c; only the fp32 summation order differs (as it does run to
// run in the reference, whose accumulation is atomicAdd too).
//
// Two forward algorithms:
//   direct : one lane per (point, rotation), 48 hardware fp32 global atomics per
//            in-bounds vote, hipMemsetAsync before and a normalise pass after.
//            This is the reference's algorithm re-parallelised over N*R lanes
//            instead of N threads (79 blocks at N=80k cannot fill 256 CUs).
//   tiles  : on-chip accumulation.  Every vote of a point has the same y, so points
//            are counting-sorted by their vote's y cell (80k keys, not 9.6M).  One
//            workgroup of eight waves owns a 16 x 32-cell (x,z) tile of ONE y plane:
//            six channels of 64-bit fixed-point accumulators, one survivor list, the
//            waves' vote queues and the rotation table - 68 KB of LDS, two workgroups
//            per CU.  It works through the points of y-bins {y-1, y} (the records
//            streamed, or this tile's work lists on large grids) in rounds of three
//            phases over ONE survivor list of the workgroup: cull (ring-vs-tile test,
//            ballot + mbcnt, one LDS reservation per hand-out), arcs (one survivor per
//            lane, workgroup scan of the arc lengths), expand (survivors x rotations
//            split evenly over all lanes, votes that land in the tile wave-compacted
//            into a queue and drained 64 at a time with LDS integer atomics).  The
//            tile is then normalised and stored once: no memset, no global atomics,
//            no second pass over the 63 MB grid.
#include "cv_common.h"

#include <atomic>
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <vector>

namespace {

struct F3 { float x, y, z; };
struct I3 { int x, y, z; };

// ---------------------------------------------------------------------------
// rotation table: (cos, sin)(i * (2*3.141592654f / R)), theta in fp32 exactly as
// hv_cuda_kernel.cu:35,37, cos/sin correctly rounded (see oracle/hv_oracle.c).
// Cached per (device, R); built once on the host.
// ---------------------------------------------------------------------------
std::mutex g_tab_mu;
std::unordered_map<uint64_t, float2*> g_tabs;

int get_rot_table(int num_rots, const float2** out) {
    int dev = 0;
    CV_HIP_CHECK(hipGetDevice(&dev));
    const uint64_t key = (uint64_t(uint32_t(dev)) << 32) | uint32_t(num_rots);
    std::lock_guard<std::mutex> lk(g_tab_mu);
    auto it = g_tabs.find(key);
    if (it != g_tabs.end()) { *out = it->second; return CV_OK; }
    std::vector<float2> h(num_rots);
    const float rot_interval = 2 * 3.141592654f / num_rots;
    for (int i = 0; i < num_rots; ++i) {
        const float theta = i * rot_interval;
        h[i].x = (float)std::cos((double)theta);
        h[i].y = (float)std::sin((double)theta);
    }
    float2* d = nullptr;
    CV_HIP_CHECK(hipMalloc(&d, sizeof(float2) * num_rots));
    CV_HIP_CHECK(hipMemcpy(d, h.data(), sizeof(float2) * num_rots, hipMemcpyHostToDevice));
    g_tabs[key] = d;
    *out = d;
    return CV_OK;
}

// ---------------------------------------------------------------------------
// shared per-vote geometry (hv_cuda_kernel.cu:38-47)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float grid_pos(float p, float off, float corner, float res) {
    return ((p + off) - corner) / res;
}

// ---------------------------------------------------------------------------
// min / max of points (hv_cuda_kernel.cu:129)
// ---------------------------------------------------------------------------
constexpr int MM_BLOCKS = 256;

__global__ __launch_bounds__(256) void minmax_partial(const float* __restrict__ pts, int64_t n,
                                                      float* __restrict__ part) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = pts[i * 3 + k];
            mn[k] = fminf(mn[k], v);
            mx[k] = fmaxf(mx[k], v);
        }
    }
    __shared__ float s[6][256];
#pragma unroll
    for (int k = 0; k < 3; ++k) { s[k][threadIdx.x] = mn[k]; s[3 + k][threadIdx.x] = mx[k]; }
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s[k][threadIdx.x] = fminf(s[k][threadIdx.x], s[k][threadIdx.x + st]);
                s[3 + k][threadIdx.x] = fmaxf(s[3 + k][threadIdx.x], s[3 + k][threadIdx.x + st]);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = s[threadIdx.x][0];
}

// zero_word / fill7f: words of the scene call's next stages initialised by this one-workgroup launch (the range flag := 0, the
// eight bound words of the row sort := 0x7f7f7f7f) instead of two fill launches of their own
__global__ __launch_bounds__(256) void minmax_final(const float* __restrict__ part, int nblocks,
                                                    float* __restrict__ out, int* __restrict__ zero_word = nullptr,
                                                    int* __restrict__ fill7f = nullptr) {
    if (zero_word && threadIdx.x == 32) *zero_word = 0;
    if (fill7f && threadIdx.x >= 64 && threadIdx.x < 72) fill7f[threadIdx.x - 64] = 0x7f7f7f7f;
    __shared__ float s[6][256];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = threadIdx.x; b < nblocks; b += 256)
        for (int k = 0; k < 3; ++k) {
            mn[k] = fminf(mn[k], part[b * 6 + k]);
            mx[k] = fmaxf(mx[k], part[b * 6 + 3 + k]);
        }
    for (int k = 0; k < 3; ++k) { s[k][threadIdx.x] = mn[k]; s[3 + k][threadIdx.x] = mx[k]; }
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st)
            for (int k = 0; k < 3; ++k) {
                s[k][threadIdx.x] = fminf(s[k][threadIdx.x], s[k][threadIdx.x + st]);
                s[3 + k][threadIdx.x] = fmaxf(s[3 + k][threadIdx.x], s[3 + k][threadIdx.x + st]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) out[threadIdx.x] = s[threadIdx.x][0];
}

// Per-scene row ranges and bounds of a batched coordinate set (cv_detect_scenes_f32): one workgroup per scene, ONE launch.
// The batch column is expected non-decreasing: the first row with a batch index >= key is found by a 1024-ary search (every
// thread probes one row of the open interval per round: three rounds cover 2^30 rows).  Scene b's rows are [lower(b),
// lower(b + 1)) - the same search gives b's end and b + 1's start, so the ranges tile [lower(0), lower(B)) by construction.
// The workgroup then checks that every row of its range carries b and reduces min / max of the points over it (min and max
// are exact: the same values minmax_partial / minmax_final give for the scene alone).  out: 16 words per scene.
constexpr int SB_T = 1024;
constexpr int SB_WORDS = 16;

__device__ __forceinline__ int64_t batch_lower_bound(const int32_t* __restrict__ coords4, int64_t n, int key) {
    int64_t lo = 0, hi = n;          // rows below lo are < key, rows from hi on are >= key (for a sorted column)
    while (lo < hi) {
        const int64_t chunk = (hi - lo + SB_T - 1) / SB_T;
        const int64_t p = lo + (int64_t)threadIdx.x * chunk;
        const int c = __syncthreads_count(p < hi && coords4[p * 4] < key);
        if (c == 0) hi = lo;
        else {
            const int64_t first_false = lo + (int64_t)c * chunk;
            lo = lo + (int64_t)(c - 1) * chunk + 1;
            hi = first_false < hi ? first_false : hi;
        }
    }
    return lo;
}

__global__ __launch_bounds__(SB_T) void scene_bounds(const int32_t* __restrict__ coords4, const float* __restrict__ pts,
                                                     int64_t n, int B, int32_t* __restrict__ out, int* __restrict__ zero_word,
                                                     int* __restrict__ fill7f) {
    const int b = blockIdx.x;
    if (b == 0) {        // (what minmax_final initialises for the scene call's next stages)
        if (zero_word && threadIdx.x == 32) *zero_word = 0;
        if (fill7f && threadIdx.x >= 64 && threadIdx.x < 72) fill7f[threadIdx.x - 64] = 0x7f7f7f7f;
    }
    const int64_t first = batch_lower_bound(coords4, n, b), end = batch_lower_bound(coords4, n, b + 1);
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = (b == 0 && first != 0) || (b == B - 1 && end != n) || end < first;
    // four rows per thread and round, their sixteen loads issued together (one workgroup walks the whole scene: a round is a
    // memory round trip); a row index beyond the range is clamped to its last row, which changes neither min, max nor the check
    for (int64_t i0 = first + threadIdx.x; i0 < end; i0 += 4 * SB_T) {
        int bt[4];
        float v[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = i0 + u * SB_T < end ? i0 + u * SB_T : end - 1;
            bt[u] = coords4[i * 4];
#pragma unroll
            for (int k = 0; k < 3; ++k) v[u][k] = pts[i * 3 + k];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            bad |= bt[u] != b;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                mn[k] = fminf(mn[k], v[u][k]);
                mx[k] = fmaxf(mx[k], v[u][k]);
            }
        }
    }
    __shared__ float s[6][SB_T];
#pragma unroll
    for (int k = 0; k < 3; ++k) { s[k][threadIdx.x] = mn[k]; s[3 + k][threadIdx.x] = mx[k]; }
    const int any_bad = __syncthreads_or(bad);
    for (int st = SB_T / 2; st > 0; st >>= 1) {
        if (threadIdx.x < st) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s[k][threadIdx.x] = fminf(s[k][threadIdx.x], s[k][threadIdx.x + st]);
                s[3 + k][threadIdx.x] = fmaxf(s[3 + k][threadIdx.x], s[3 + k][threadIdx.x + st]);
            }
        }
        __syncthreads();
    }
    int32_t* o = out + b * SB_WORDS;
    if (threadIdx.x < 6) o[2 + threadIdx.x] = __float_as_int(s[threadIdx.x][0]);
    if (threadIdx.x == 6) o[0] = (int32_t)first;
    if (threadIdx.x == 7) o[1] = (int32_t)end;
    if (threadIdx.x == 8) o[8] = any_bad ? 1 : 0;
}

// ---------------------------------------------------------------------------
// direct algorithm
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hv_fwd_direct(
    const float* __restrict__ pts, const float* __restrict__ xyz, const float* __restrict__ scl,
    const float* __restrict__ obj, int64_t n, int R, float res, F3 corner, I3 dims,
    const float2* __restrict__ tab, float* __restrict__ g_obj, float* __restrict__ g_rot,
    float* __restrict__ g_scale) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= n * R) return;
    const int64_t c = t / R;
    const int i = (int)(t - c * R);
    const float s0 = scl[c * 3 + 0], s1 = scl[c * 3 + 1], s2 = scl[c * 3 + 2];
    const float cx = xyz[c * 3 + 0] * s0, cy = xyz[c * 3 + 1] * s1, cz = xyz[c * 3 + 2] * s2;
    const float2 cs = tab[i];
    const float ox = (-cs.x) * cx + cs.y * cz;
    const float oy = -cy;
    const float oz = (-cs.y) * cx - cs.x * cz;
    const float gx = grid_pos(pts[c * 3 + 0], ox, corner.x, res);
    const float gy = grid_pos(pts[c * 3 + 1], oy, corner.y, res);
    const float gz = grid_pos(pts[c * 3 + 2], oz, corner.z, res);
    if (gx < 0 || gy < 0 || gz < 0 || gx >= (float)(dims.x - 1) || gy >= (float)(dims.y - 1) ||
        gz >= (float)(dims.z - 1))
        return;
    const int fx = (int)gx, fy = (int)gy, fz = (int)gz;
    const float rx = gx - floorf(gx), ry = gy - floorf(gy), rz = gz - floorf(gz);
    const float wx[2] = {1.f - rx, rx}, wy[2] = {1.f - ry, ry}, wz[2] = {1.f - rz, rz};
    const float ob = obj[c];
    const int Y = dims.y, Z = dims.z;
#pragma unroll
    for (int bx = 0; bx < 2; ++bx)
#pragma unroll
        for (int by = 0; by < 2; ++by)
#pragma unroll
            for (int bz = 0; bz < 2; ++bz) {
                const float w = wx[bx] * wy[by] * wz[bz] * ob;
                const int64_t cell = ((int64_t)(fx + bx) * Y + (fy + by)) * Z + (fz + bz);
                unsafeAtomicAdd(&g_obj[cell], w);
                unsafeAtomicAdd(&g_rot[cell * 2 + 0], w * cs.x);
                unsafeAtomicAdd(&g_rot[cell * 2 + 1], w * cs.y);
                unsafeAtomicAdd(&g_scale[cell * 3 + 0], w * s0);
                unsafeAtomicAdd(&g_scale[cell * 3 + 1], w * s1);
                unsafeAtomicAdd(&g_scale[cell * 3 + 2], w * s2);
            }
}

// hv_cuda_kernel.cu:100-119, coalesced along Z (flat cell index).
__global__ __launch_bounds__(256) void hv_normalise(const float* __restrict__ g_obj,
                                                    float* __restrict__ g_rot,
                                                    float* __restrict__ g_scale, int64_t cells) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= cells) return;
    const double d = (double)g_obj[i] + 1e-7;
    float2 r = reinterpret_cast<float2*>(g_rot)[i];
    r.x = (float)((double)r.x / d);
    r.y = (float)((double)r.y / d);
    reinterpret_cast<float2*>(g_rot)[i] = r;
#pragma unroll
    for (int j = 0; j < 3; ++j) g_scale[i * 3 + j] = (float)((double)g_scale[i * 3 + j] / d);
}

// ---------------------------------------------------------------------------
// tiles algorithm
// ---------------------------------------------------------------------------
// Tile = TX x 32 cells of one y plane, TW waves per workgroup.
// 16 x 32 cells / 8 waves (68 KB of LDS, two workgroups per CU): the fastest shape one scene in flight (0.36 ms) and with
// scenes in flight (profiles/r3/vote_tile_sweep.txt).  Round 3 found it giving WRONG cells - a few dozen cells of one
// (plane, tile), weight moved between neighbouring cells - in about a third of the launches that ran while fp16 / bf16
// matrix-core convolutions of OTHER streams were resident on the same CU (tests/test_concurrency_gpu.py).  The cause is
// not in this kernel: on gfx950 a `v_pk_add_f32 ... op_sel:[0,1] op_sel_hi:[1,0]` - what the SLP vectoriser makes of the
// 2-D rotation of the offset below - returns wrong results while another wave of the CU issues
// v_mfma_f32_32x32x16_{f16,bf16} / 16x16x32_f16 (never next to the fp32 or the 32x32x8 f16 MFMA; pinned with synthetic
// co-resident loads and an instruction-class checker: profiles/vote_hammer_probe.py, op_check_probe.py,
// microbench/lds_hammer.hip, r3/vote_concurrency_findings.txt).  The whole library is built without packed fp32
// instructions now (csrc/build.py); with that every tile shape is exact under the same load (0 of 400 / 0 of 4800).
constexpr int TX = 16, TZ = 32, TCELLS = TX * TZ;   // tile cells in x / z: the fastest shape of the sweep above; TZ = 32 is built into acc_idx
constexpr int TW = 8;        // waves per workgroup: same sweep (profiles/r3/vote_tile_sweep.txt), 68 KB of LDS = two workgroups per CU
constexpr int LQ = TW * 64;  // surviving records per round of the workgroup: one per lane
constexpr int CULL_BATCH = 4;     // 64-record chunks a wave culls per hand-out: their loads in flight at once, cull 22 % -> 9 % of
                                  // the wave time against one chunk per hand-out (profiles/r8/vote_dense.txt)
static_assert(CULL_BATCH >= 1 && CULL_BATCH <= 8, "one carry bit and one record index per sub-chunk and lane");
constexpr int VQ = 128;      // vote queue entries per wave
constexpr int MAX_R_TILES = 256;
static_assert(MAX_R_TILES <= TW * 64, "the rotation table is staged by one load per lane");
constexpr int LIST_CHUNK = 16;    // list entries of a chunk, the unit the parts of a hot (tile, plane) interleave by: four chunks
                                  // fill a wave's hand-out (the value of the round-3 work lists; never swept on its own)
static_assert(64 % LIST_CHUNK == 0, "a wave takes 64 / LIST_CHUNK list chunks per hand-out, one entry per lane");
// what a queued vote (TileShared::vq_rec: entry | rot << 9 | (lx + 1) << 17 | (lz + 1) << 23) and drain64 assume
static_assert(LQ <= 512, "the list entry of a queued vote has 9 bits");
static_assert(MAX_R_TILES <= 256, "the rotation of a queued vote has 8 bits");
static_assert(TX + 1 < 64 && TZ + 1 < 64, "lx + 1 and lz + 1 of a queued vote have 6 bits each");
static_assert(TZ == 32, "acc_idx splits a cell index by >> 5 and & 31");

// y cell of every vote of a point (theta-independent: offset.y = -corr.y, :38-39).
// Global atomics on a few hot addresses serialise at ~11 ns each on MI355X (measured: 80k
// atomics over 88 counters = 142 us), so bins are aggregated per workgroup in LDS first.
constexpr int LIST_CHUNK_RECORDS = 1024;     // records of one y-bin per work-list workgroup (hv_list_pass)
constexpr int PREP_MAX_Y = 4096;
constexpr int PREP_THREADS = 1024;

// Category axis (cv_hv_forward_cat_f32): launch dimension y is the category.  Every category has its own workspace carve
// with the layout of category 0's (records, counters, lists, partials), `ws` bytes behind the previous one, its predictions
// `n` points and its grids `cells` cells behind the previous category's.  The scan points, the grid origin and shape and
// the rotation table are shared.  K = 1 (cv_hv_forward_f32) has blockIdx.y = 0: every offset is zero.
struct CatStride { int64_t ws, n, cells; };
template <class T>
__device__ __forceinline__ T* cat_ws(T* p, int64_t bytes) {
    return (T*)((const char*)p + (int64_t)blockIdx.y * bytes);
}
template <class T>
__device__ __forceinline__ T* cat_el(T* p, int64_t elems) {
    return p + (int64_t)blockIdx.y * elems;
}

// (the bodies of the vote's kernels are device functions: the category kernels and the scene kernels - further down, behind
// TilesLayout - differ only in where a workgroup finds its pointers)
__device__ __forceinline__ void prep_count_body(
    const float* __restrict__ pts, const float* __restrict__ xyz, const float* __restrict__ scl,
    int64_t n, float res, float corner_y, int Y, int* __restrict__ fy_out, int* __restrict__ ycount) {
    __shared__ int lh[PREP_MAX_Y];
    const bool use_lds = Y <= PREP_MAX_Y;
    if (use_lds) {
        for (int i = threadIdx.x; i < Y; i += PREP_THREADS) lh[i] = 0;
        __syncthreads();
    }
    const int64_t c = blockIdx.x * (int64_t)PREP_THREADS + threadIdx.x;
    if (c < n) {
        const float cy = xyz[c * 3 + 1] * scl[c * 3 + 1];
        const float gy = grid_pos(pts[c * 3 + 1], -cy, corner_y, res);
        int fy = -1;
        if (gy >= 0 && gy < (float)(Y - 1)) fy = (int)gy;
        fy_out[c] = fy;
        if (fy >= 0) atomicAdd(use_lds ? &lh[fy] : &ycount[fy], 1);
    }
    if (use_lds) {
        __syncthreads();
        for (int i = threadIdx.x; i < Y; i += PREP_THREADS)
            if (lh[i]) atomicAdd(&ycount[i], lh[i]);
    }
}
__global__ __launch_bounds__(PREP_THREADS) void hv_prep_count(
    const float* __restrict__ pts, const float* __restrict__ xyz, const float* __restrict__ scl,
    int64_t n, float res, float corner_y, int Y, int* __restrict__ fy_out, int* __restrict__ ycount, CatStride ks) {
    xyz = cat_el(xyz, 3 * ks.n); scl = cat_el(scl, 3 * ks.n);
    fy_out = cat_ws(fy_out, ks.ws); ycount = cat_ws(ycount, ks.ws);
    prep_count_body(pts, xyz, scl, n, res, corner_y, Y, fy_out, ycount);
}

// exclusive scan of ycount[Y] -> ystart[Y+1], cursor[Y] (single workgroup)
// Hough peaks concentrate votes: the hottest (tile, plane) of an 80k scene receives ~27x the mean and
// would take 0.3 ms on one CU.  Planes whose two y-bins hold many points are therefore split into
// up to MAX_PARTS workgroups per tile (disjoint record chunks), merged by the last arriver.
constexpr int PART_RECORDS = 4096;   // records per part, the floor of cv_hv_set_part_records: fastest with one scene in flight
constexpr int MAX_PARTS = 8;         // against 2048 / 8192 records and 16 parts (profiles/r1/vote_tile_sweep.txt, r5/vote_parts.txt)

// (round 3: the three scans used to be Hillis-Steele passes over 1024 LDS slots with two workgroup barriers per step -
// sixty barriers for Y = 88 bins, 7.5 us; they are independent, so three waves run one wave-level scan each: 64 bins per step)
template <class V, class E>
__device__ __forceinline__ int wave_excl_scan(int Y, V value, E emit) {
    const int lane = threadIdx.x & 63;
    int carry = 0;
    for (int base = 0; base < Y; base += 64) {
        const int i = base + lane;
        const int v = i < Y ? value(i) : 0;
        int incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (i < Y) emit(i, carry + incl - v, v);
        carry += __shfl(incl, 63);
    }
    return carry;
}
__device__ __forceinline__ void prep_scan_body(const int* __restrict__ ycount, int Y, int* __restrict__ ystart,
                                               int* __restrict__ cursor, int* __restrict__ part_start,
                                               int4* __restrict__ q_info, int max_q, int* __restrict__ chunk_start,
                                               int* __restrict__ bin_of_chunk, int part_records) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave == 0) {
        const int total = wave_excl_scan(Y, [&](int i) { return ycount[i]; },
                                         [&](int i, int excl, int) { ystart[i] = excl; cursor[i] = excl; });
        if (lane == 0) ystart[Y] = total;
    } else if (wave == 1) {
        // streaming path (small grids): part_start[y] = exclusive scan of the number of workgroups per tile of plane y, by
        // the records of its two bins; q_info[(plane, part) slot] = (plane, part, parts of the plane, first slot of the plane),
        // nparts = -1 on the unused slots behind the last one: ONE 16-byte load in front of a tile workgroup's work (round 1: a
        // binary search over part_start, seven dependent loads; round 2: three dependent loads part_start[Y] ->
        // plane_of_q[q] -> part_start[y], part_start[y + 1])
        const int total = wave_excl_scan(Y,
            [&](int i) {
                const int n2 = (i >= 1 ? ycount[i - 1] : 0) + (i <= Y - 2 ? ycount[i] : 0);
                return min(max((n2 + part_records - 1) / part_records, 1), MAX_PARTS);
            },
            [&](int i, int excl, int v) {
                part_start[i] = excl;
                for (int p2 = 0; p2 < v; ++p2) q_info[excl + p2] = make_int4(i, p2, v, excl);
            });
        for (int q = total + lane; q < max_q; q += 64) q_info[q] = make_int4(0, 0, -1, 0);
        if (lane == 0) part_start[Y] = total;
    } else if (wave == 2) {
        // chunks of up to LIST_CHUNK_RECORDS records of one bin (the work-list passes run one workgroup per chunk)
        const int total = wave_excl_scan(Y, [&](int i) { return (ycount[i] + LIST_CHUNK_RECORDS - 1) / LIST_CHUNK_RECORDS; },
                                         [&](int i, int excl, int v) {
                                             chunk_start[i] = excl;
                                             for (int p2 = 0; p2 < v; ++p2) bin_of_chunk[excl + p2] = i;
                                         });
        if (lane == 0) chunk_start[Y] = total;
    }
}
__global__ __launch_bounds__(256) void hv_prep_scan(const int* __restrict__ ycount, int Y,
                                                    int* __restrict__ ystart,
                                                    int* __restrict__ cursor,
                                                    int* __restrict__ part_start, int4* __restrict__ q_info, int max_q,
                                                    int* __restrict__ chunk_start, int* __restrict__ bin_of_chunk,
                                                    int part_records, int64_t ks_ws) {
    ycount = cat_ws(ycount, ks_ws); ystart = cat_ws(ystart, ks_ws); cursor = cat_ws(cursor, ks_ws);
    part_start = cat_ws(part_start, ks_ws); q_info = cat_ws(q_info, ks_ws);
    chunk_start = cat_ws(chunk_start, ks_ws); bin_of_chunk = cat_ws(bin_of_chunk, ks_ws);
    prep_scan_body(ycount, Y, ystart, cursor, part_start, q_info, max_q, chunk_start, bin_of_chunk, part_records);
}

// Scatters every point with an in-bounds y into its y-bin and writes a compact SoA record
// (REC_F floats, bin order) so the tile kernel streams coalesced rows instead of gathering
// 10 scalars per point through `order[]`:
//   0 px  1 pz  2 cx  3 cz  4 ry (fractional y)  5 obj  6..8 scale  9 ux  10 uz  11 r  12 a0
// (ux,uz) = ring centre, r = ring radius in grid units and a0 = angle (seen from the ring centre)
// of the vote at rotation 0; used only for culling.
constexpr int REC_F = 13;

__device__ __forceinline__ void prep_scatter_body(
    const float* __restrict__ pts, const float* __restrict__ xyz, const float* __restrict__ scl,
    const float* __restrict__ obj, const int* __restrict__ fy_in, int64_t n, int Y, float res,
    F3 corner, int* __restrict__ cursor, float* __restrict__ rec, int64_t rec_stride) {
    __shared__ int lh[PREP_MAX_Y];     // per-workgroup count, then the workgroup's base in the bin
    const bool use_lds = Y <= PREP_MAX_Y;
    const int64_t c = blockIdx.x * (int64_t)PREP_THREADS + threadIdx.x;
    const int fy = c < n ? fy_in[c] : -1;
    int pos = -1;
    if (!use_lds) {
        if (fy >= 0) pos = atomicAdd(&cursor[fy], 1);
    } else {
        for (int i = threadIdx.x; i < Y; i += PREP_THREADS) lh[i] = 0;
        __syncthreads();
        int rank = 0;
        if (fy >= 0) rank = atomicAdd(&lh[fy], 1);
        __syncthreads();
        for (int i = threadIdx.x; i < Y; i += PREP_THREADS)
            if (lh[i]) lh[i] = atomicAdd(&cursor[i], lh[i]);
        __syncthreads();
        if (fy >= 0) pos = lh[fy] + rank;
    }
    if (pos < 0) return;
    const float px = pts[c * 3 + 0], py = pts[c * 3 + 1], pz = pts[c * 3 + 2];
    const float s0 = scl[c * 3 + 0], s1 = scl[c * 3 + 1], s2 = scl[c * 3 + 2];
    const float cx = xyz[c * 3 + 0] * s0, cy = xyz[c * 3 + 1] * s1, cz = xyz[c * 3 + 2] * s2;
    const float gy = grid_pos(py, -cy, corner.y, res);
    float* r = rec + pos;
    r[0 * rec_stride] = px;
    r[1 * rec_stride] = pz;
    r[2 * rec_stride] = cx;
    r[3 * rec_stride] = cz;
    r[4 * rec_stride] = gy - floorf(gy);
    r[5 * rec_stride] = obj[c];
    r[6 * rec_stride] = s0;
    r[7 * rec_stride] = s1;
    r[8 * rec_stride] = s2;
    r[9 * rec_stride] = (px - corner.x) / res;
    r[10 * rec_stride] = (pz - corner.z) / res;
    r[11 * rec_stride] = sqrtf(cx * cx + cz * cz) / res;
    // vote(theta) = u - r (cos(theta + phi), sin(theta + phi)) with (cx, cz) = r (cos phi, sin phi)
    r[12 * rec_stride] = atan2f(cz, cx) + 3.14159265f;
}
__global__ __launch_bounds__(PREP_THREADS) void hv_prep_scatter(
    const float* __restrict__ pts, const float* __restrict__ xyz, const float* __restrict__ scl,
    const float* __restrict__ obj, const int* __restrict__ fy_in, int64_t n, int Y, float res,
    F3 corner, int* __restrict__ cursor, float* __restrict__ rec, int64_t rec_stride, CatStride ks) {
    xyz = cat_el(xyz, 3 * ks.n); scl = cat_el(scl, 3 * ks.n); obj = cat_el(obj, ks.n);
    fy_in = cat_ws(fy_in, ks.ws); cursor = cat_ws(cursor, ks.ws); rec = cat_ws(rec, ks.ws);
    prep_scatter_body(pts, xyz, scl, obj, fy_in, n, Y, res, corner, cursor, rec, rec_stride);
}


// ---- per-(y-bin, tile) work lists (round 3) ------------------------------------------------------------------------
// Every tile of a plane used to stream ALL records of its two y-bins and cull them (ring vs rectangle, then the arc):
// 66 tiles x 88 planes x ~1800 records at 80k points, 41 % of the kernel's wave time and most of its VALU work
// (profiles/r3/vote_pmc_sq_before.txt).  The test depends on (record, tile) only, so it is done ONCE: one workgroup per
// y-bin walks its records twice (count, then fill) over the tiles in the ring's bounding box and writes, per (bin, tile),
// the list of (record, first rotation, arc length) entries the tile kernel expands.  Lists live in one bump-allocated
// array; when it overflows (rings that cover the whole grid) a flag sends the tile kernel back to the streaming path.
constexpr int LIST_MAX_TILES = 4096;
struct RingArc { bool keep; int a_start, a_len; };
__device__ __forceinline__ bool ring_touches(float ux, float uz, float r, float xlo, float xhi, float zlo, float zhi,
                                             float& dxn, float& dzn) {
    const float slack = 0.05f;
    dxn = fmaxf(0.f, fmaxf(xlo - ux, ux - xhi));
    dzn = fmaxf(0.f, fmaxf(zlo - uz, uz - zhi));
    const float dxf = fmaxf(fabsf(ux - xlo), fabsf(ux - xhi));
    const float dzf = fmaxf(fabsf(uz - zlo), fabsf(uz - zhi));
    const float dmin = sqrtf(dxn * dxn + dzn * dzn), dmax = sqrtf(dxf * dxf + dzf * dzf);
    const float tol = slack + 1e-5f * (r + fabsf(ux) + fabsf(uz));
    return (r >= dmin - tol) && (r <= dmax + tol);
}
// rotations whose vote can fall in the rectangle: it subtends an arc seen from the ring centre unless the centre is
// (nearly) inside it
__device__ __forceinline__ void ring_arc(float ux, float uz, float a0, int R, float xlo, float xhi, float zlo, float zhi,
                                         float dxn, float dzn, int& a_start, int& a_len) {
    a_start = 0;
    a_len = R;
    if (dxn + dzn > 0.5f) {
        const float b0 = atan2f(0.5f * (zlo + zhi) - uz, 0.5f * (xlo + xhi) - ux);
        float lo = 0.f, hi = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float d = atan2f(((k & 2) ? zhi : zlo) - uz, ((k & 1) ? xhi : xlo) - ux) - b0;
            d -= 6.28318531f * rintf(d * 0.159154943f);
            lo = fminf(lo, d);
            hi = fmaxf(hi, d);
        }
        const float inv_step = (float)R * 0.159154943f;          // 1 / rot_interval
        float first = (b0 + lo - a0) * inv_step - 2.f;           // 2 steps of slack per side
        const int len = (int)((hi - lo) * inv_step) + 6;
        first -= (float)R * floorf(first / (float)R);
        a_start = min(max((int)first, 0), R - 1);
        a_len = min(len, R);
    }
}

// Launches over CHUNKS of up to 1024 records of one y-bin (a bin per workgroup left the floor's bin - a quarter of an 80k
// scene - to one workgroup: 200 us):
//   hv_list_pass<false>  per (bin, tile): the summed arc lengths of the rings that reach the tile (tile_w: what the work
//                        queue sizes the parts of a hot tile with) and, when lists are wanted, the entry counts
//                        (atomicAdd on the (bin, tile) total returns the chunk's first slot inside that list)
//   hv_list_scan         lists only, one workgroup: exclusive scan of the entry counts (list starts, overflow flag)
//   hv_list_pass<true>   lists only, the same walk again: entry -> list_start + chunk slot + LDS rank
// chunk_start[Y + 1] / bin_of_chunk[] come from hv_prep_scan.
template <bool FILL>
__device__ __forceinline__ void list_pass_body(const int* __restrict__ ystart, const int* __restrict__ chunk_start,
                                               const int* __restrict__ bin_of_chunk, int Y, const float* __restrict__ rec,
                                               int64_t rec_stride, int R, int tiles_x, int tiles_z,
                                               const int* __restrict__ list_ctl, int* __restrict__ list_cnt,
                                               const int* __restrict__ list_start, int* __restrict__ chunk_off,
                                               int2* __restrict__ entries, int* __restrict__ tile_w, int want_lists) {
    __shared__ int cnt[LIST_MAX_TILES];
    __shared__ int wsum[FILL ? 1 : LIST_MAX_TILES];
    const int ntiles = tiles_x * tiles_z;
    const int c = blockIdx.x;
    if (c >= chunk_start[Y]) return;
    if (FILL && list_ctl[1] != 0) return;             // overflow: the tile kernel streams the bins
    const int bin = bin_of_chunk[c];
    const int idx = ystart[bin] + (c - chunk_start[bin]) * LIST_CHUNK_RECORDS + (int)threadIdx.x;
    const int end = ystart[bin + 1];
    for (int t = threadIdx.x; t < ntiles; t += 1024) {
        cnt[t] = FILL ? list_start[(int64_t)bin * ntiles + t] + chunk_off[(int64_t)c * ntiles + t] : 0;
        if (!FILL) wsum[t] = 0;
    }
    __syncthreads();
    if (idx < end) {
        const float ux = rec[9 * rec_stride + idx], uz = rec[10 * rec_stride + idx], r = rec[11 * rec_stride + idx];
        const float a0 = rec[12 * rec_stride + idx];
        // tiles whose rectangle [x0 - 1, x0 + TX] x [z0 - 1, z0 + TZ] can meet the ring's bounding box (+ slack)
        const float ext = r + 2.f + 1e-5f * (r + fabsf(ux) + fabsf(uz));
        const int tx0 = max(0, (int)floorf((ux - ext - (float)TX) / (float)TX));
        const int tx1 = min(tiles_x - 1, (int)floorf((ux + ext + 1.f) / (float)TX));
        const int tz0 = max(0, (int)floorf((uz - ext - (float)TZ) / (float)TZ));
        const int tz1 = min(tiles_z - 1, (int)floorf((uz + ext + 1.f) / (float)TZ));
        for (int tx = tx0; tx <= tx1; ++tx)
            for (int tz = tz0; tz <= tz1; ++tz) {
                const float xlo = (float)(tx * TX - 1), xhi = (float)(tx * TX + TX), zlo = (float)(tz * TZ - 1),
                            zhi = (float)(tz * TZ + TZ);
                float dxn, dzn;
                if (!ring_touches(ux, uz, r, xlo, xhi, zlo, zhi, dxn, dzn)) continue;
                int a_start, a_len;
                ring_arc(ux, uz, a0, R, xlo, xhi, zlo, zhi, dxn, dzn, a_start, a_len);
                const int t = tx * tiles_z + tz;
                if (FILL) {
                    const int p = atomicAdd(&cnt[t], 1);
                    entries[p] = make_int2(idx, a_start | (a_len << 16));
                } else {
                    if (want_lists) atomicAdd(&cnt[t], 1);
                    atomicAdd(&wsum[t], a_len);
                }
            }
    }
    if (FILL) return;
    __syncthreads();
    for (int t = threadIdx.x; t < ntiles; t += 1024) {
        if (want_lists) chunk_off[(int64_t)c * ntiles + t] = cnt[t] ? atomicAdd(&list_cnt[(int64_t)bin * ntiles + t], cnt[t]) : 0;
        if (wsum[t]) atomicAdd(&tile_w[(int64_t)bin * ntiles + t], wsum[t]);
    }
}
template <bool FILL>
__global__ __launch_bounds__(1024) void hv_list_pass(const int* __restrict__ ystart, const int* __restrict__ chunk_start,
                                                     const int* __restrict__ bin_of_chunk, int Y,
                                                     const float* __restrict__ rec, int64_t rec_stride, int R, int tiles_x,
                                                     int tiles_z, const int* __restrict__ list_ctl, int* __restrict__ list_cnt,
                                                     const int* __restrict__ list_start, int* __restrict__ chunk_off,
                                                     int2* __restrict__ entries, int* __restrict__ tile_w, int want_lists,
                                                     int64_t ks_ws) {
    ystart = cat_ws(ystart, ks_ws); chunk_start = cat_ws(chunk_start, ks_ws); bin_of_chunk = cat_ws(bin_of_chunk, ks_ws);
    rec = cat_ws(rec, ks_ws); list_ctl = cat_ws(list_ctl, ks_ws); list_cnt = cat_ws(list_cnt, ks_ws);
    list_start = cat_ws(list_start, ks_ws); chunk_off = cat_ws(chunk_off, ks_ws); entries = cat_ws(entries, ks_ws);
    tile_w = cat_ws(tile_w, ks_ws);
    list_pass_body<FILL>(ystart, chunk_start, bin_of_chunk, Y, rec, rec_stride, R, tiles_x, tiles_z, list_ctl, list_cnt, list_start,
                         chunk_off, entries, tile_w, want_lists);
}

// list_ctl[0] = total entries, list_ctl[1] = overflow flag (zeroed by the caller's fill)
__device__ __forceinline__ void list_scan_body(const int* __restrict__ list_cnt, int Y, int ntiles, long long list_cap,
                                               int* __restrict__ list_ctl, int* __restrict__ list_start) {
    __shared__ int s[1024];
    __shared__ long long carry_s;      // 64 bits: a total past 2^31 must raise the overflow flag, not wrap
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    const int total_lists = Y * ntiles;
    for (int base = 0; base < total_lists; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < total_lists ? list_cnt[i] : 0;
        s[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int t = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0;
            __syncthreads();
            s[threadIdx.x] += t;
            __syncthreads();
        }
        const long long incl = (long long)s[threadIdx.x] + carry_s;
        if (i < total_lists) list_start[i] = incl - v < 0x7fffffffll ? (int)(incl - v) : 0x7fffffff;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) { list_ctl[0] = carry_s < 0x7fffffffll ? (int)carry_s : 0x7fffffff; list_ctl[1] = carry_s > list_cap ? 1 : 0; }
}
__global__ __launch_bounds__(1024) void hv_list_scan(const int* __restrict__ list_cnt, int Y, int ntiles, long long list_cap,
                                                     int* __restrict__ list_ctl, int* __restrict__ list_start, int64_t ks_ws) {
    list_cnt = cat_ws(list_cnt, ks_ws); list_ctl = cat_ws(list_ctl, ks_ws); list_start = cat_ws(list_start, ks_ws);
    list_scan_body(list_cnt, Y, ntiles, list_cap, list_ctl, list_start);
}

// ---- work queue of the tile kernel (round 3) -----------------------------------------------------------------------
// The launch used to hold (plane, part) x tile workgroups with the parts of a plane sized by the RECORDS of its two
// bins.  The time of the kernel was the time of its hottest tile: 1 % of the (plane, tile) pairs of an 80k scene
// receive 20 % of the votes (up to 26 x the mean of the non-empty ones) while a plane's record count says nothing about
// where its rings meet.  The queue holds one item per (plane, tile) that receives nothing (it only writes zeros) and
// ceil(weight / PART_VOTES) items for the others, weight = summed arc lengths of the rings that reach the tile in the
// plane's two bins (hv_list_pass<false>); parts merge through `partials` slots handed out by the same scan.
//   item = (plane, tile, part | parts << 8, first partial slot of the (plane, tile))
constexpr int PART_VOTES = 32768;    // arc steps per part: 64 per lane of the workgroup (set with the round-3 queue on the 300k-point
                                     // scene, 2.01 -> 1.32 ms for the vote stage; never swept on its own)
constexpr int QUEUE_MAX_PARTS = 32;

__device__ __forceinline__ void build_queue_body(const int* __restrict__ tile_w, int Y, int ntiles, int max_items, int max_slots,
                                                 int* __restrict__ list_ctl /*[2] = items*/, int4* __restrict__ items) {
    __shared__ unsigned long long s[1024];
    __shared__ unsigned long long carry_s;
    const int total = Y * ntiles;
    // pass 0 sizes the parts by weight; when the items or the partial slots would not fit, pass 1 gives every tile one part
    for (int pass = 0; pass < 2; ++pass) {
        if (threadIdx.x == 0) carry_s = 0ull;
        __syncthreads();
        for (int base = 0; base < total; base += 1024) {
            const int i = base + threadIdx.x;
            int parts = 0, y = 0, t = 0;
            if (i < total) {
                y = i / ntiles; t = i - y * ntiles;
                const long long w = (long long)(y >= 1 ? tile_w[(int64_t)(y - 1) * ntiles + t] : 0) +
                                    (long long)(y <= Y - 2 ? tile_w[(int64_t)y * ntiles + t] : 0);
                parts = w == 0 ? 0 : (pass ? 1 : (int)min((long long)QUEUE_MAX_PARTS, (w + PART_VOTES - 1) / PART_VOTES));
            }
            // items in the high word, partial slots (tiles with more than one part) in the low word
            const unsigned long long v = i < total ? (((unsigned long long)max(parts, 1) << 32) | (unsigned)(parts > 1 ? parts : 0)) : 0ull;
            s[threadIdx.x] = v;
            __syncthreads();
            for (int off = 1; off < 1024; off <<= 1) {
                const unsigned long long x = (int)threadIdx.x >= off ? s[threadIdx.x - off] : 0ull;
                __syncthreads();
                s[threadIdx.x] += x;
                __syncthreads();
            }
            const unsigned long long excl = s[threadIdx.x] + carry_s - v;
            const int item0 = (int)(excl >> 32), slot0 = (int)(excl & 0xffffffffull);
            if (i < total && item0 + max(parts, 1) <= max_items && slot0 + (parts > 1 ? parts : 0) <= max_slots) {
                if (parts == 0) items[item0] = make_int4(y, t, 0, 0);
                for (int p2 = 0; p2 < parts; ++p2) items[item0 + p2] = make_int4(y, t, p2 | (parts << 8), slot0);
            }
            __syncthreads();
            if (threadIdx.x == 1023) carry_s = s[1023] + carry_s;
            __syncthreads();
        }
        const int n_items = (int)(carry_s >> 32), n_slots = (int)(carry_s & 0xffffffffull);
        if (n_items <= max_items && n_slots <= max_slots) {
            if (threadIdx.x == 0) list_ctl[2] = n_items;
            return;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) list_ctl[2] = min(total, max_items);     // (total <= max_items by construction)
}
__global__ __launch_bounds__(1024) void hv_build_queue(const int* __restrict__ tile_w, int Y, int ntiles, int max_items,
                                                       int max_slots, int* __restrict__ list_ctl /*[2] = items*/,
                                                       int4* __restrict__ items, int64_t ks_ws) {
    tile_w = cat_ws(tile_w, ks_ws); list_ctl = cat_ws(list_ctl, ks_ws); items = cat_ws(items, ks_ws);
    build_queue_body(tile_w, Y, ntiles, max_items, max_slots, list_ctl, items);
}

__device__ __forceinline__ int lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// LDS atomic add rates on gfx950 (lane-ops/clk/CU, measured: profiles/microbench/lds_atomic_rate.hip):
// f32 0.33, f64 3.1, u64 5.6, u32 7.4.  (Round 2's ablation - 0.68 ms -> 0.25 ms without the atomics - also removed the
// conversions in front of them; by the round-6 counters the kernel issues vector ALU instructions 80 % of its time and waits
// for LDS 4.5 % of its wave cycles: LABNOTES round 8.)  The objectness channel - the one the decode thresholds and takes argmax of, and the
// one that defines which cells are touched at all - accumulates in f64 (exact sums of the fp32 contributions).
// The five quotient numerators (rot cos/sin, scale xyz) accumulate in 64-bit FIXED POINT with ds_add_u64: every
// fp32 contribution is rounded once to a multiple of 2^-36 (1.5e-11; |sum| < 1.3e8 per cell and channel) and
// integer addition is exact and order independent, so all six sums are reproducible run to run; the rounding is
// 1e-11 relative on cells with weight >= 1 and only matters on cells whose total weight is below ~1e-6 (their
// rot / scale quotients lose digits; the reference's own fp32 atomics lose ~1e-7 relative per add everywhere).
constexpr double FX_SCALE = 68719476736.0;            // 2^36
constexpr double FX_MAGIC = 6755399441055744.0;       // 1.5 * 2^52: (x*2^36 + MAGIC) has round(x*2^36) in its low bits
// round(v * 2^36) as a two's-complement word
template <bool SMALL>
__device__ __forceinline__ unsigned long long fx_from_float(float v) {
    if (SMALL) {                              // the magic-number conversion holds for |v * 2^36| < 2^51
        const double d = __builtin_fma((double)v, FX_SCALE, FX_MAGIC);
        return (unsigned long long)__double_as_longlong(d) - (unsigned long long)__double_as_longlong(FX_MAGIC);
    }
    // huge contributions (a diverged scale head): exact up to 6e7, clamped beyond
    return (unsigned long long)__double2ll_rn((double)fminf(fmaxf(v, -6.0e7f), 6.0e7f) * FX_SCALE);
}
template <bool SMALL>
__device__ __forceinline__ void lds_add(unsigned long long* p, float v) {
    __hip_atomic_fetch_add(p, fx_from_float<SMALL>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ double fx_value(unsigned long long q) { return (double)(long long)q * (1.0 / FX_SCALE); }
// The objectness weight - the channel that is thresholded, arg-maxed and defines the touched-cell set - accumulated in
// f64 until round 3: sums of fp32 contributions spanning more than 53 bits are not exact in f64, so the LDS atomics'
// order reached the last bits and, once in ~1600 runs of one scene, a cell on an fp32 rounding boundary changed the
// greedy walk (tests/test_concurrency_gpu.py found it).  It now uses the same 2^-36 fixed point as the numerators
// (integer addition: exact, order independent, bit-reproducible) with ONE extra rule: a non-zero contribution never rounds
// to zero (it adds one quantum, 1.5e-11), so a cell is non-zero exactly when the reference's fp32 sum is.
template <bool SMALL>
__device__ __forceinline__ void lds_add_obj(unsigned long long* p, float v) {
    unsigned long long q = fx_from_float<SMALL>(v);
    if (q == 0ull && v != 0.f) q = v > 0.f ? 1ull : ~0ull;
    __hip_atomic_fetch_add(p, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// LDS layout of the tile accumulators: word of (channel ch, cell (cx, cz)) = ch * ACC_CH + cx * ACC_PITCH + cz.
// With a pitch of 32 words the bank of a cell (64 banks x 4 B, a 64-bit word takes two) depended on cz alone, so the
// lanes of one atomic instruction whose votes spread along x - a ring crossing the tile, the cluster around a Hough
// peak - serialised on one bank.  Pitch 40: +1 in z = 2 banks, +1 in x = 80 = 16 banks (mod 64): every cell of a 4x4
// neighbourhood has its own bank.  Vote op 0.512 -> 0.447 ms on the network's predictions (pitches 34 / 36 / 40 / 44:
// 0.457 / 0.445 / 0.447 / 0.443).  Measured and dropped: walking the (corner, channel) slots of a vote in a per-lane
// rotated order so that lanes voting into the SAME cell hit different words in different banks at any one instruction -
// 0.62 ms (same-address lanes of one ds_add are evidently merged more cheaply than 24 rotated selects cost), rotating
// the channel order only - 0.45 / 0.47 ms (no gain).
constexpr int ACC_PITCH = TZ + 8, ACC_CH = TX * ACC_PITCH + 4;
__device__ __forceinline__ int acc_idx(int ch, int cell) { return ch * ACC_CH + (cell >> 5) * ACC_PITCH + (cell & 31); }

// The channel set of a tile launch.  The rot / scale quotients are read in ONE place of the pipeline - the decode's compaction,
// at cells with objectness >= thresh_high, 0.12 % of an 80k scene's grid - so a caller that only decodes runs two launches over
// the same work items instead of VOTE_FULL:
//   VOTE_FULL   all six channels, all three grids (cv_hv_forward_f32)
//   VOTE_OBJ    the objectness channel alone; stores g_obj and, per (plane, tile), the bounding box of its cells >= thresh
//   VOTE_PEAKS  the five numerators, only in the tiles that hold such a cell and only for corners inside that box; stores
//               g_rot / g_scale at the cells >= thresh, dividing by the float VOTE_OBJ stored
// Every sum is an integer, so the quotients of the second launch are the bits VOTE_FULL writes.
constexpr int VOTE_FULL = 0, VOTE_OBJ = 1, VOTE_PEAKS = 2;
constexpr int vote_channels(int mode) { return mode == VOTE_FULL ? 6 : (mode == VOTE_OBJ ? 1 : 5); }
// cells >= thresh of one (plane, tile), tile-local and inclusive; x0 > x1: none
struct HotBox { int x0, x1, z0, z1; };

template <int MODE>
struct TileSharedT {
    static constexpr int ACC_WORDS = vote_channels(MODE) * ACC_CH;
    unsigned long long acc[ACC_WORDS];   // VOTE_FULL: channel 0: objectness weight, 1..5: rot.cos, rot.sin, scale.xyz (VOTE_OBJ:
                                         // channel 0 alone, VOTE_PEAKS: the five numerators as channels 0..4) - all in 2^-36 fixed point
    float pq[MODE == VOTE_OBJ ? 6 : 9][LQ];   // px, pz, cx, cz, wy, obj, s0, s1, s2 of the round's surviving records (workgroup-wide list)
    int arc_start[LQ];         // phase A: record index | bin << 31; from phase B on: first rotation whose vote can reach the tile
    int arc_cum[LQ];           // (list mode, phase A: the entry's packed arc) inclusive prefix sum of the arc lengths
    uint32_t vq_rec[TW][VQ];   // entry | rot<<9 | (lx+1)<<17 | (lz+1)<<23
    float vq_rx[TW][VQ];
    float vq_rz[TW][VQ];
    float2 tab[MAX_R_TILES];
    int next_chunk[2];         // dynamic hand-out of 64-record chunks of the two y-bins to the waves
    int wtot[TW];              // summed arc lengths of each wave's 64 list entries (workgroup scan of phase B)
    int list_len;              // entries reserved in the list this round (may run past LQ: the surplus is carried over)
    int more;                  // a wave stopped for lack of room: another round follows
};

template <bool SMALL, int MODE>
__device__ __forceinline__ void drain_vote(TileSharedT<MODE>& sh, int lx, int lz, float rx, float rz, float wy, float ob,
                                           float s0, float s1, float s2, float2 cs, HotBox box) {
    const float wx[2] = {1.f - rx, rx}, wz[2] = {1.f - rz, rz};
#pragma unroll
    for (int bx = 0; bx < 2; ++bx)
#pragma unroll
        for (int bz = 0; bz < 2; ++bz) {
            const int cxl = lx + bx, czl = lz + bz;
            if (MODE == VOTE_PEAKS) {
                if (cxl < box.x0 || cxl > box.x1 || czl < box.z0 || czl > box.z1) continue;
            } else {
                if (cxl < 0 || cxl >= TX || czl < 0 || czl >= TZ) continue;
            }
            // hv_cuda_kernel.cu:52-59 order: ((wx*wy)*wz)*objness
            const float w = wx[bx] * wy * wz[bz] * ob;
            unsigned long long* a = sh.acc + cxl * ACC_PITCH + czl;
            if (MODE != VOTE_PEAKS) lds_add_obj<SMALL>(a, w);
            if (MODE == VOTE_OBJ) continue;
            if (MODE == VOTE_FULL) a += ACC_CH;
            lds_add<SMALL>(a, w * cs.x);
            lds_add<SMALL>(a + ACC_CH, w * cs.y);
            lds_add<SMALL>(a + 2 * ACC_CH, w * s0);
            lds_add<SMALL>(a + 3 * ACC_CH, w * s1);
            lds_add<SMALL>(a + 4 * ACC_CH, w * s2);
        }
}

template <int MODE>
__device__ __forceinline__ void drain64(TileSharedT<MODE>& sh, int wave, int slot, bool active, HotBox box) {
    float rx = 0.f, rz = 0.f, wy = 0.f, ob = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
    float2 cs = make_float2(0.f, 0.f);
    int lx = 0, lz = 0;
    // (round 6, VERDICT r5 item 3b, profiles/r6/vote_bank_bucket.txt: dealing the 64 votes of a drain to the two 32-lane halves by
    // their rank among the lanes of the same bank pair - five ballots for the same-bank mask, two for the positions, one
    // ds_permute - took SQ_LDS_BANK_CONFLICT from 3.98e7 to 3.41e7 per launch (45.6 % -> 41.1 % of SQ_LDS_IDX_ACTIVE) and the LDS
    // wait cycles down by a third, and cost 7 % more wave cycles: 0.357 against 0.333 ms, 591 against 598 scenes/s.  Removed.
    // profiles/vote_run_pricing.py has the ceilings: a PERFECT permutation inside the 64 saves 23 % of the bank cycles, merging
    // runs of votes that keep their floor cell 28 % of the atomics (mean run length 1.38).)
    if (active) {
        const uint32_t rec = sh.vq_rec[wave][slot];
        rx = sh.vq_rx[wave][slot]; rz = sh.vq_rz[wave][slot];
        const int e = rec & 511, rot = (rec >> 9) & 255;
        lx = (int)((rec >> 17) & 63) - 1; lz = (int)((rec >> 23) & 63) - 1;
        wy = sh.pq[4][e]; ob = sh.pq[5][e];
        if constexpr (MODE != VOTE_OBJ) {
            s0 = sh.pq[6][e]; s1 = sh.pq[7][e]; s2 = sh.pq[8][e];
            cs = sh.tab[rot];
        }
    }
    // every contribution of a vote is bounded by |obj| * max(1, |scale|) (the trilinear weights are <= 1); the
    // wave takes the fast fixed-point conversion unless one of its 64 votes could exceed its range.  (VOTE_OBJ has s = 0: the
    // objectness contribution is bounded by |obj| alone, and inside the fast conversion's range both conversions round v * 2^36
    // to the nearest integer, ties to even - the same word whichever the wave takes.)
    const bool small = fabsf(ob) * fmaxf(1.f, fmaxf(fabsf(s0), fmaxf(fabsf(s1), fabsf(s2)))) < 16384.f;
    if (__all(small)) {
        if (active) drain_vote<true, MODE>(sh, lx, lz, rx, rz, wy, ob, s0, s1, s2, cs, box);
    } else {
        if (active) drain_vote<false, MODE>(sh, lx, lz, rx, rz, wy, ob, s0, s1, s2, cs, box);
    }
}

__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// atan2 for the arc of rotations a tile can receive from a ring (conservative culling only: every vote is placed by the
// exact fp32 sequence afterwards).  |error| < 2e-4 rad against 2 rotation steps of slack per side (0.1 rad at 120 rotations,
// 0.05 at 256): the libm atan2f calls (five per kept record) were a third of the tile kernel's vector instructions.
__device__ __forceinline__ float arc_atan2(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float a = fminf(ax, ay) * __builtin_amdgcn_rcpf(fmaxf(fmaxf(ax, ay), 1e-30f));
    const float q = a * a;
    float r = ((-0.0464964749f * q + 0.15931422f) * q - 0.327622764f) * q * a + a;
    r = ay > ax ? 1.57079637f - r : r;
    r = x < 0.f ? 3.14159274f - r : r;
    return y < 0.f ? -r : r;
}

// A second conservative arc, for rings that the corner arc serves badly: a centre inside the rectangle (or within half a
// cell) gets all R rotations and 54 % of the expanded items of an 80k scene come from such rings, although a ring larger
// than the tile spends most of its circumference outside (profiles/r8/vote_chunk_pricing.txt: 2.49 items per in-tile vote,
// 1.38 with this arc in the model).  Beyond the edge line with outward normal at angle k pi/2 and distance d < r from the centre
// the ring runs for the angles within acos(d / r) of the normal.  Neighbouring outside arcs that overlap merge into runs; the
// complement of the LONGEST run is one interval that holds every vote inside the rectangle.  Everything errs to the safe
// side: the rectangle grown by `slack`, every outside arc shortened by 0.01 rad per side (the atan2 polynomial is good to
// 2e-4), arcs linked only where the shortened ones still overlap, rings under two cells left to the corner arc (there the
// rounding of the centre is not small against the radius), and the usual two rotation steps of slack per side.
__device__ __forceinline__ void edge_arc(float ux, float uz, float r, float a0, int R, float xlo, float xhi, float zlo,
                                         float zhi, int& a_start, int& a_len) {
    if (!(r >= 2.f)) return;
    const float slack = 0.05f, half_pi = 1.57079637f, two_pi = 6.28318531f;
    const float d4[4] = {xhi - ux, zhi - uz, ux - xlo, uz - zlo};          // outward normals at 0, pi/2, pi, 3 pi/2
    const float inv_r = 1.f / r;
    float h[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t = (d4[k] + slack) * inv_r;
        const float hk = arc_atan2(sqrtf(fmaxf(1.f - t * t, 0.f)), t) - 0.01f;      // acos(t), t <= -1: pi
        h[k] = (t < 1.f && hk > 0.f) ? hk : -1.f;                                   // -1: the ring does not cross this line
    }
    float best = 0.f, best_end = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float lo = -h[k], hi = h[k];
        bool ok = h[k] > 0.f;
        if (ok && hi - lo > best) { best = hi - lo; best_end = (float)k * half_pi + hi; }
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            const float hp = h[(k + j - 1) & 3], hn = h[(k + j) & 3];
            ok = ok && hn > 0.f && hp + hn >= half_pi;
            if (ok) {
                lo = fminf(lo, (float)j * half_pi - hn);
                hi = fmaxf(hi, (float)j * half_pi + hn);
                if (hi - lo > best) { best = hi - lo; best_end = (float)k * half_pi + hi; }
            }
        }
    }
    const float inside = fmaxf(two_pi - best, 0.f);
    const float inv_step = (float)R * 0.159154943f;
    const int len = (int)(inside * inv_step) + 6;
    if (len < a_len) {
        float first = (best_end - a0) * inv_step - 2.f;
        first -= (float)R * floorf(first / (float)R);
        a_start = min(max((int)first, 0), R - 1);
        a_len = len;
    }
}

// One work item (plane y, tile, part of nparts) of a tile launch; the pointers are the category's own.  VOTE_FULL ignores the
// last three arguments in front of `tab`:
//   hot / thresh  VOTE_OBJ writes, VOTE_PEAKS reads: hot[plane * ntiles + tile] = the HotBox of the cells whose stored objectness is
//                 >= thresh - the float and the comparison of the decode's compaction.  Every record is written by every VOTE_OBJ
//                 launch (by the workgroup that stores the tile), so nothing of it survives a call.
//   hot_items     VOTE_OBJ appends, VOTE_PEAKS walks: the work items (plane, tile, part | parts << 8, first partial slot) of the
//                 (plane, tile) pairs whose box is not empty; its length is the word arrivals[Y * ntiles] (TilesLayout).
template <bool QUEUE, int MODE>
__device__ __forceinline__ void hv_tile_item(
    int y, int tile, int part, int nparts, int slot0, int slot_stride,
    int R, float res, F3 corner, I3 dims,
    const int* __restrict__ ystart, const float* __restrict__ rec,
    int64_t rec_stride, int tiles_x, int tiles_z, unsigned long long* __restrict__ partials,
    int* __restrict__ arrivals, float* __restrict__ g_obj, float* __restrict__ g_rot,
    float* __restrict__ g_scale, const int* __restrict__ list_ctl, const int* __restrict__ list_start, const int* __restrict__ list_cnt,
    const int2* __restrict__ entries, int list_mode /* 1: stream the bins, 2: work lists */,
    int4* __restrict__ hot, float thresh, int4* __restrict__ hot_items, const float2* __restrict__ tab) {
    constexpr int NCH = vote_channels(MODE);
    __shared__ TileSharedT<MODE> sh;
    __shared__ int last_flag;
    __shared__ int hot_lds[MODE == VOTE_OBJ ? 4 : 1];      // VOTE_OBJ: x lo / hi, z lo / hi of the tile's cells >= thresh
    const int X = dims.x, Y = dims.y, Z = dims.z;
    const int ntiles = tiles_x * tiles_z;
    const int x0 = (tile / tiles_z) * TX, z0 = (tile % tiles_z) * TZ;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // VOTE_PEAKS: the cells of this (plane, tile) that the decode can read; none (most tiles): nothing to do, for every part alike
    HotBox box{0, TX - 1, 0, TZ - 1};
    if (MODE == VOTE_PEAKS) {
        const int4 h = hot[y * ntiles + tile];
        box = HotBox{h.x, h.y, h.z, h.w};
        if (box.x0 > box.x1) return;
    }
    if (nparts == 0) {
        // nothing votes into this tile of this plane: zeros straight to the grids (no accumulators, no barriers)
        const int nx0 = min(TX, X - x0), nz0 = min(TZ, Z - z0);
        for (int i = threadIdx.x; i < TCELLS; i += TW * 64) {
            const int lx = i / TZ, lz = i % TZ;
            if (lx < nx0 && lz < nz0) {
                const int64_t cell = ((int64_t)(x0 + lx) * Y + y) * Z + z0 + lz;
                if (MODE != VOTE_PEAKS) g_obj[cell] = 0.f;
                if (MODE != VOTE_OBJ) {      // (VOTE_PEAKS gets here with thresh <= 0 only: every cell of the tile counts)
                    reinterpret_cast<float2*>(g_rot)[cell] = make_float2(0.f, 0.f);
                    g_scale[cell * 3 + 0] = 0.f; g_scale[cell * 3 + 1] = 0.f; g_scale[cell * 3 + 2] = 0.f;
                }
            }
        }
        if (MODE == VOTE_OBJ && threadIdx.x == 0) {
            hot[y * ntiles + tile] = 0.f >= thresh ? make_int4(0, nx0 - 1, 0, nz0 - 1) : make_int4(TX, -1, TZ, -1);
            if (0.f >= thresh) hot_items[atomicAdd(&arrivals[Y * ntiles], 1)] = make_int4(y, tile, 0, slot0);
        }
        return;
    }
    // list_mode 2: work lists of this tile in the two y-bins (hv_list_pass; list_ctl[1] != 0: they overflowed, stream the
    // bins instead)
    const bool use_list = QUEUE && list_mode == 2 && list_ctl[1] == 0;      // (the queue launch is the list launch)
    int lbeg[2] = {0, 0}, llen[2] = {0, 0};
    if (use_list) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int s = y - 1 + k;
            if (s >= 0 && s <= Y - 2) {
                lbeg[k] = list_start[(int64_t)s * ntiles + tile];
                llen[k] = list_cnt[(int64_t)s * ntiles + tile];
            }
        }
    }

    // first and last record (list entry) of the two bins and the rotation table: loads issued before the accumulators are
    // zeroed, so that their latency passes under the zeroing and not in front of phase A
    int bin_beg[2], bin_end[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int s = y - 1 + k;
        const bool valid = s >= 0 && s <= Y - 2;
        bin_beg[k] = !valid ? 0 : (use_list ? lbeg[k] : ystart[s]);
        bin_end[k] = !valid ? 0 : (use_list ? lbeg[k] + llen[k] : ystart[s + 1]);
    }
    const float2 tab_mine = (int)threadIdx.x < R ? tab[threadIdx.x] : make_float2(0.f, 0.f);      // (R <= MAX_R_TILES <= TW * 64)
    for (int i = threadIdx.x; i < TileSharedT<MODE>::ACC_WORDS; i += TW * 64) sh.acc[i] = 0ull;
    if ((int)threadIdx.x < R) sh.tab[threadIdx.x] = tab_mine;
    if (threadIdx.x < 2) sh.next_chunk[threadIdx.x] = 0;
    if (threadIdx.x == 2) { sh.list_len = 0; sh.more = 0; }
    if (MODE == VOTE_OBJ && threadIdx.x >= 4 && threadIdx.x < 8)      // (read behind the barriers of the tail)
        hot_lds[threadIdx.x - 4] = (threadIdx.x & 1) ? -1 : (threadIdx.x == 4 ? TX : TZ);
    __syncthreads();

    // a vote at grid position g touches cells floor(g), floor(g)+1, so it reaches this
    // tile iff g in [x0-1, x0+TX) x [z0-1, z0+TZ); slack covers fp32 rounding of the test.
    // (VOTE_PEAKS: the hot box in place of the tile - the cull, the arcs and the vote test below all take this rectangle)
    const float slack = 0.05f;
    const float xlo = MODE == VOTE_PEAKS ? (float)(x0 + box.x0 - 1) : (float)(x0 - 1),
                xhi = MODE == VOTE_PEAKS ? (float)(x0 + box.x1 + 1) : (float)(x0 + TX),
                zlo = MODE == VOTE_PEAKS ? (float)(z0 + box.z0 - 1) : (float)(z0 - 1),
                zhi = MODE == VOTE_PEAKS ? (float)(z0 + box.z1 + 1) : (float)(z0 + TZ);
    int vq_len = 0;   // wave-uniform

    // Rounds of three phases over ONE survivor list of the workgroup (until round 8 every wave culled a 64-record chunk,
    // kept ~5 records of it and paid the arc, the scan, the search and a queue flush for those five):
    //   A  the waves take chunks of both y-bins from the shared counters, run only the ring-vs-rectangle test and append the
    //      kept records (ballot, mbcnt, one LDS reservation per wave and hand-out) to the list;
    //   B  one survivor per lane: arc, record fields, workgroup-wide inclusive scan of the arc lengths;
    //   C  the round's items split evenly over all lanes of the workgroup, one binary search per lane, votes queued per
    //      wave and drained 64 at a time; a wave flushes its queue once per round.
    // A round ends when the list cannot take another full chunk.  Survivors of a chunk that found the list full stay in the
    // wave's registers (c_*) and open its next round: no record is dropped or taken twice.
    const int per = use_list ? LIST_CHUNK : 64;           // records (list entries) of a chunk: the unit of the part split
    int sb = 0;                               // bin (0: y - 1, 1: y) this wave takes chunks of; wave-uniform
    // A wave takes CULL_BATCH chunks per hand-out and has the loads of all of them in flight at once: phase A is a chain of
    // (LDS counter, global loads, test, LDS reservation) per hand-out and nothing of the workgroup overlaps it.
    // carried survivors: bit j of c_mask = this lane's record of sub-chunk j (c_idx[j]; list mode: packed arc c_arc), c_k their bin
    int c_mask = 0, c_idx[CULL_BATCH], c_arc = 0, c_k = 0;
#pragma unroll
    for (int j = 0; j < CULL_BATCH; ++j) c_idx[j] = 0;
    // appends the kept records of a hand-out behind ONE reservation; returns the bits the list had no room for
    auto append = [&](int mask, const int (&idx)[CULL_BATCH], int arc, int k) -> int {
        int tot = 0, before[CULL_BATCH];
#pragma unroll
        for (int j = 0; j < CULL_BATCH; ++j) {
            const uint64_t m = __ballot((mask >> j) & 1);
            before[j] = tot + lanes_below(m);
            tot += __popcll(m);
        }
        if (tot == 0) return 0;
        int p0 = 0;
        if (lane == 0) p0 = atomicAdd(&sh.list_len, tot);
        p0 = __builtin_amdgcn_readfirstlane(p0);
#pragma unroll
        for (int j = 0; j < CULL_BATCH; ++j) {
            const int pos = p0 + before[j];
            if (((mask >> j) & 1) && pos < LQ) {
                sh.arc_start[pos] = idx[j] | (int)((unsigned)k << 31);
                if (use_list) sh.arc_cum[pos] = arc;
                mask &= ~(1 << j);
            }
        }
        return mask;
    };

    for (;;) {
        // ---- phase A: cull chunks into the list
        bool more = false;                    // wave-uniform: this wave stopped for lack of room
        if (__ballot(c_mask != 0) != 0) {
            c_mask = append(c_mask, c_idx, c_arc, c_k);
            more = __ballot(c_mask != 0) != 0;
        }
        while (!more && sb < 2) {
            if (bin_beg[sb] >= bin_end[sb]) { ++sb; continue; }
            const int len = __builtin_amdgcn_readfirstlane(
                __hip_atomic_load(&sh.list_len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
            if (len > LQ - 64) { more = true; break; }       // no room for another full chunk: the round ends
            // waves take chunks from a shared counter: a wave whose chunks are slow to cull takes fewer of them
            const int take = use_list ? 64 / LIST_CHUNK : CULL_BATCH;
            int c = 0;
            if (lane == 0) c = atomicAdd(&sh.next_chunk[sb], take);
            c = __builtin_amdgcn_readfirstlane(c);
            const int end = bin_end[sb];
            if (bin_beg[sb] + (c * nparts + part) * per >= end) { ++sb; continue; }
            int idx[CULL_BATCH], mask = 0, arc = 0;
#pragma unroll
            for (int j = 0; j < CULL_BATCH; ++j) idx[j] = 0;
            if (use_list) {
                // 64 / LIST_CHUNK chunks of LIST_CHUNK entries: one entry per lane
                const int e = bin_beg[sb] + ((c + lane / LIST_CHUNK) * nparts + part) * LIST_CHUNK + lane % LIST_CHUNK;
                if (e < end) {
                    const int2 en = entries[e];
                    idx[0] = en.x;
                    arc = en.y;
                    mask = 1;
                }
            } else {
                float ux[CULL_BATCH], uz[CULL_BATCH], r[CULL_BATCH];
#pragma unroll
                for (int j = 0; j < CULL_BATCH; ++j) {
                    idx[j] = bin_beg[sb] + ((c + j) * nparts + part) * 64 + lane;
                    const bool in = idx[j] < end;
                    ux[j] = in ? rec[9 * rec_stride + idx[j]] : 0.f;
                    uz[j] = in ? rec[10 * rec_stride + idx[j]] : 0.f;
                    r[j] = in ? rec[11 * rec_stride + idx[j]] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < CULL_BATCH; ++j) {
                    // conservative ring-vs-rectangle test in grid units
                    const float dxn = fmaxf(0.f, fmaxf(xlo - ux[j], ux[j] - xhi));
                    const float dzn = fmaxf(0.f, fmaxf(zlo - uz[j], uz[j] - zhi));
                    const float dxf = fmaxf(fabsf(ux[j] - xlo), fabsf(ux[j] - xhi));
                    const float dzf = fmaxf(fabsf(uz[j] - zlo), fabsf(uz[j] - zhi));
                    const float dmin = sqrtf(dxn * dxn + dzn * dzn), dmax = sqrtf(dxf * dxf + dzf * dzf);
                    const float tol = slack + 1e-5f * (r[j] + fabsf(ux[j]) + fabsf(uz[j]));
                    const bool keep = idx[j] < end && (r[j] >= dmin - tol) && (r[j] <= dmax + tol);
                    mask |= (int)keep << j;
                }
            }
            c_mask = append(mask, idx, arc, sb);
            if (__ballot(c_mask != 0) != 0) {
#pragma unroll
                for (int j = 0; j < CULL_BATCH; ++j) c_idx[j] = idx[j];
                c_arc = arc; c_k = sb;
                more = true;
            }
        }
        if (more && lane == 0) sh.more = 1;
        __syncthreads();
        const int n = min(sh.list_len, LQ);
        const bool again = sh.more != 0;      // (implies n > 0: room runs out only in a list that holds entries)
        if (n == 0) break;

        // ---- phase B: one survivor per lane
        const int p = threadIdx.x;
        int a_start = 0, a_len = 0;
        if (p < n) {
            const int w = sh.arc_start[p];
            const int idx = w & 0x7fffffff;
            if (use_list) {
                const int arc = sh.arc_cum[p];
                a_start = arc & 0xffff;
                a_len = arc >> 16;
            } else {
                // rotations whose vote can fall in the rectangle: the rectangle subtends an arc
                // [b0+lo, b0+hi] seen from the ring centre unless the centre is (nearly) inside it
                const float ux = rec[9 * rec_stride + idx], uz = rec[10 * rec_stride + idx];
                const float dxn = fmaxf(0.f, fmaxf(xlo - ux, ux - xhi));
                const float dzn = fmaxf(0.f, fmaxf(zlo - uz, uz - zhi));
                a_len = R;
                if (dxn + dzn > 0.5f) {
                    const float b0 = arc_atan2(0.5f * (zlo + zhi) - uz, 0.5f * (xlo + xhi) - ux);
                    float lo = 0.f, hi = 0.f;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float d = arc_atan2(((k & 2) ? zhi : zlo) - uz, ((k & 1) ? xhi : xlo) - ux) - b0;
                        d -= 6.28318531f * rintf(d * 0.159154943f);
                        lo = fminf(lo, d);
                        hi = fmaxf(hi, d);
                    }
                    const float a0 = rec[12 * rec_stride + idx];
                    const float inv_step = (float)R * 0.159154943f;          // 1 / rot_interval
                    float first = (b0 + lo - a0) * inv_step - 2.f;           // 2 steps of slack per side
                    const int len = (int)((hi - lo) * inv_step) + 6;
                    first -= (float)R * floorf(first / (float)R);
                    a_start = min(max((int)first, 0), R - 1);
                    a_len = min(len, R);
                }
                edge_arc(ux, uz, rec[11 * rec_stride + idx], rec[12 * rec_stride + idx], R, xlo, xhi, zlo, zhi, a_start, a_len);
            }
            const float ry = rec[4 * rec_stride + idx];
            sh.pq[0][p] = rec[0 * rec_stride + idx];
            sh.pq[1][p] = rec[1 * rec_stride + idx];
            sh.pq[2][p] = rec[2 * rec_stride + idx];
            sh.pq[3][p] = rec[3 * rec_stride + idx];
            sh.pq[4][p] = (w < 0) ? (1.f - ry) : ry;       // bin y : bin y - 1
            sh.pq[5][p] = rec[5 * rec_stride + idx];
            if constexpr (MODE != VOTE_OBJ) {
                sh.pq[6][p] = rec[6 * rec_stride + idx];
                sh.pq[7][p] = rec[7 * rec_stride + idx];
                sh.pq[8][p] = rec[8 * rec_stride + idx];
            }
            sh.arc_start[p] = a_start;
        }
        // inclusive scan of the arc lengths in list order: per wave, then over the wave totals
        int cum = a_len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(cum, off);
            if (lane >= off) cum += t;
        }
        if (lane == 63) sh.wtot[wave] = cum;
        __syncthreads();
        if (threadIdx.x == 0) { sh.list_len = 0; sh.more = 0; }      // (every lane has read both; next written after the
                                                                     // barrier that ends the round)
        int items = 0;
#pragma unroll
        for (int w = 0; w < TW; ++w) {
            const int t = sh.wtot[w];
            if (w < wave) cum += t;
            items += t;
        }
        if (p < n) sh.arc_cum[p] = cum;
        __syncthreads();

        // ---- phase C: slice j walks items [j*S, (j+1)*S): at any step the lanes of a wave sit on different arcs
        // (different cells -> few same-address LDS atomic collisions), and a lane only advances along its arc, so the
        // (entry, step) pair is found by ONE binary search per round.
        const int S = (items + LQ - 1) / LQ;
        const int slice = wave * 64 + lane;          // a wave walks one contiguous run of the list (interleaved slices: no
                                                     // faster, profiles/r8/vote_dense.txt)
        int it0 = slice * S;
        const int it1 = min(it0 + S, items);
        int e = 0;
        {
            int lo = 0, hi = n - 1;                      // smallest e with cum[e] > it0
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sh.arc_cum[mid] > it0) hi = mid; else lo = mid + 1;
            }
            e = lo;
        }
        int e_end = it0 < items ? sh.arc_cum[e] : 0;          // first item of the next entry
        int rot = 0;
        // the entry's point stays in registers while the lane walks its arc (4 LDS reads per entry instead of
        // per step: the LDS pipe is what the expansion shares with the atomics)
        float epx = 0.f, epz = 0.f, ecx = 0.f, ecz = 0.f;
        if (it0 < items) {
            const int e_beg = e > 0 ? sh.arc_cum[e - 1] : 0;
            rot = sh.arc_start[e] + (it0 - e_beg);
            if (rot >= R) rot -= R;
            epx = sh.pq[0][e]; epz = sh.pq[1][e];
            ecx = sh.pq[2][e]; ecz = sh.pq[3][e];
        }
        for (int step = 0; step < S; ++step, ++it0) {
            bool isvote = false;
            uint32_t vrec = 0;
            float rx = 0, rz = 0;
            if (it0 < it1) {
                if (it0 == e_end) {                      // next arc
                    ++e;
                    e_end = sh.arc_cum[e];
                    rot = sh.arc_start[e];
                    epx = sh.pq[0][e]; epz = sh.pq[1][e];
                    ecx = sh.pq[2][e]; ecz = sh.pq[3][e];
                }
                const float2 cs = sh.tab[rot];
                const float ox = (-cs.x) * ecx + cs.y * ecz;
                const float oz = (-cs.y) * ecx - cs.x * ecz;
                const float gx = grid_pos(epx, ox, corner.x, res);
                const float gz = grid_pos(epz, oz, corner.z, res);
                if (gx >= 0 && gz >= 0 && gx < (float)(X - 1) && gz < (float)(Z - 1)) {
                    const int lx = (int)gx - x0, lz = (int)gz - z0;
                    // (VOTE_PEAKS: one of the four corners in the hot box)
                    if (MODE == VOTE_PEAKS ? (lx >= box.x0 - 1 && lx <= box.x1 && lz >= box.z0 - 1 && lz <= box.z1)
                                           : (lx >= -1 && lx < TX && lz >= -1 && lz < TZ)) {
                        isvote = true;
                        rx = gx - floorf(gx);
                        rz = gz - floorf(gz);
                        vrec = (uint32_t)e | ((uint32_t)rot << 9) | ((uint32_t)(lx + 1) << 17) |
                               ((uint32_t)(lz + 1) << 23);
                    }
                }
                if (++rot == R) rot = 0;
            }
            const uint64_t mv = __ballot(isvote);
            if (isvote) {
                const int q = vq_len + lanes_below(mv);
                sh.vq_rec[wave][q] = vrec;
                sh.vq_rx[wave][q] = rx;
                sh.vq_rz[wave][q] = rz;
            }
            vq_len += __popcll(mv);
            wave_sync_lds();
            if (vq_len >= 64) {
                vq_len -= 64;
                drain64<MODE>(sh, wave, vq_len + lane, true, box);
            }
        }
        // queued votes index this round's list entries: flush before the list is overwritten
        if (vq_len > 0) {
            drain64<MODE>(sh, wave, lane, lane < vq_len, box);
            vq_len = 0;
        }
        wave_sync_lds();
        if (!again) break;
        __syncthreads();
    }
    __syncthreads();

    if (nparts > 1) {
        // publish this part's tile as the raw 2^-36 fixed-point words, the last arriver adds the parts as integers: the
        // merged sums are the same bits whichever records landed in whichever part (until round 4 the parts went through
        // fp32, so the last bit of a hot cell depended on the atomic order of the scatter that fills the parts)
        // plain stores -> per-wave vmcnt(0) -> barrier -> one-lane agent release -> ticket.
        // (a slot has room for six channels in every mode: VOTE_OBJ and VOTE_PEAKS use the first one / five of the same slots,
        // one launch after the other)
        unsigned long long* mine = partials + ((int64_t)slot0 + (int64_t)part * slot_stride) * (6 * TCELLS);
        for (int i = threadIdx.x; i < NCH * TCELLS; i += TW * 64) mine[i] = sh.acc[acc_idx(i / TCELLS, i % TCELLS)];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const int old = __hip_atomic_fetch_add(&arrivals[y * ntiles + tile], 1, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
            last_flag = old == nparts - 1;
            if (last_flag) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            // the VOTE_PEAKS launch behind this one counts its arrivals in the same word: back to zero once all have arrived
            if (MODE == VOTE_OBJ && last_flag)
                __hip_atomic_store(&arrivals[y * ntiles + tile], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (!last_flag) return;
        const unsigned long long* base = partials + (int64_t)slot0 * (6 * TCELLS);
        for (int i = threadIdx.x; i < NCH * TCELLS; i += TW * 64) {
            unsigned long long sum = 0ull;
            for (int p2 = 0; p2 < nparts; ++p2) sum += base[(int64_t)p2 * slot_stride * (6 * TCELLS) + i];
            sh.acc[acc_idx(i / TCELLS, i % TCELLS)] = sum;
        }
        __syncthreads();
    }

    // fused normalise (hv_cuda_kernel.cu:112-117) + single store of the tile.  The weight the
    // reference divides by is the fp32 grid value, so round the double sum to float first.
    const int nx = min(TX, X - x0), nz = min(TZ, Z - z0);
    if constexpr (MODE == VOTE_OBJ) {
        // the objectness grid, and the box of the cells the decode's compaction will take (the same float, the same comparison)
        for (int i = threadIdx.x; i < TCELLS; i += TW * 64) {
            const int lx = i / TZ, lz = i % TZ;
            if (lx < nx && lz < nz) {
                const float v = (float)fx_value(sh.acc[acc_idx(0, i)]);
                g_obj[((int64_t)(x0 + lx) * Y + y) * Z + z0 + lz] = v;
                if (v >= thresh) {
                    atomicMin(&hot_lds[0], lx); atomicMax(&hot_lds[1], lx);
                    atomicMin(&hot_lds[2], lz); atomicMax(&hot_lds[3], lz);
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            hot[y * ntiles + tile] = make_int4(hot_lds[0], hot_lds[1], hot_lds[2], hot_lds[3]);
            if (hot_lds[0] <= hot_lds[1]) {      // every part of this (plane, tile) is an item of the VOTE_PEAKS launch
                const int at = atomicAdd(&arrivals[Y * ntiles], nparts);
                for (int p2 = 0; p2 < nparts; ++p2) hot_items[at + p2] = make_int4(y, tile, p2 | (nparts << 8), slot0);
            }
        }
    } else if constexpr (MODE == VOTE_PEAKS) {
        // quotients at the cells >= thresh, by the formula below with the float the VOTE_OBJ launch stored
        for (int i = threadIdx.x; i < TCELLS; i += TW * 64) {
            const int lx = i / TZ, lz = i % TZ;
            if (lx < box.x0 || lx > box.x1 || lz < box.z0 || lz > box.z1) continue;       // (the box lies inside nx x nz)
            const int64_t cell = ((int64_t)(x0 + lx) * Y + y) * Z + z0 + lz;
            const float v = g_obj[cell];
            if (!(v >= thresh)) continue;
            const double d = (double)v + 1e-7;
#pragma unroll
            for (int j = 0; j < 2; ++j) g_rot[cell * 2 + j] = (float)((double)(float)fx_value(sh.acc[acc_idx(j, i)]) / d);
#pragma unroll
            for (int j = 0; j < 3; ++j) g_scale[cell * 3 + j] = (float)((double)(float)fx_value(sh.acc[acc_idx(2 + j, i)]) / d);
        }
    } else {
        for (int i = threadIdx.x; i < TCELLS; i += TW * 64) {
            const int lx = i / TZ, lz = i % TZ;
            if (lx < nx && lz < nz)
                g_obj[((int64_t)(x0 + lx) * Y + y) * Z + z0 + lz] = (float)fx_value(sh.acc[acc_idx(0, i)]);
        }
        for (int i = threadIdx.x; i < TCELLS * 2; i += TW * 64) {
            const int cell = i >> 1, j = i & 1;
            const int lx = cell / TZ, lz = cell % TZ;
            if (lx < nx && lz < nz) {
                const double d = (double)(float)fx_value(sh.acc[acc_idx(0, cell)]) + 1e-7;
                g_rot[(((int64_t)(x0 + lx) * Y + y) * Z + z0 + lz) * 2 + j] =
                    (float)((double)(float)fx_value(sh.acc[acc_idx(1 + j, cell)]) / d);
            }
        }
        for (int i = threadIdx.x; i < TCELLS * 3; i += TW * 64) {
            const int cell = i / 3, j = i - cell * 3;
            const int lx = cell / TZ, lz = cell % TZ;
            if (lx < nx && lz < nz) {
                const double d = (double)(float)fx_value(sh.acc[acc_idx(0, cell)]) + 1e-7;
                g_scale[(((int64_t)(x0 + lx) * Y + y) * Z + z0 + lz) * 3 + j] =
                    (float)((double)(float)fx_value(sh.acc[acc_idx(3 + j, cell)]) / d);
            }
        }
    }
}

// The launch: which item(s) a workgroup takes.  VOTE_FULL / VOTE_OBJ: one per workgroup.  QUEUE: hv_build_queue's items (large
// grids) - ONE 16-byte load says which (plane, tile, part) this is.  !QUEUE (small grids, the round-2 launch): (plane, part) x tile
// workgroups, parts by the records of the plane's bins (hv_prep_scan).  VOTE_PEAKS: PEAK_WGS workgroups stride over hot_items -
// launched one workgroup per item of the full launch it spent its time on ~8 000 workgroups that found an empty record
// (LABNOTES, vote peaks).
template <bool QUEUE, int MODE>
__device__ __forceinline__ void fwd_tiles_body(
    int R, float res, F3 corner, I3 dims, const float2* __restrict__ tab,
    const int* __restrict__ ystart, const int4* __restrict__ items, const float* __restrict__ rec,
    int64_t rec_stride, int tiles_x, int tiles_z, unsigned long long* __restrict__ partials,
    int* __restrict__ arrivals, float* __restrict__ g_obj, float* __restrict__ g_rot,
    float* __restrict__ g_scale, const int* __restrict__ list_ctl, const int* __restrict__ list_start, const int* __restrict__ list_cnt,
    const int2* __restrict__ entries, int list_mode /* 1: stream the bins, 2: work lists */,
    const int4* __restrict__ q_info, int4* __restrict__ hot, float thresh, int4* __restrict__ hot_items) {
    const int ntiles = tiles_x * tiles_z;
#define CV_TILE_ITEM_ARGS R, res, corner, dims, ystart, rec, rec_stride, tiles_x, tiles_z, partials, arrivals, g_obj, g_rot, g_scale, \
                          list_ctl, list_start, list_cnt, entries, list_mode, hot, thresh, hot_items
    if (MODE == VOTE_PEAKS) {
        const int count = arrivals[dims.y * ntiles];
        if ((int)blockIdx.x >= count) return;
        for (int i = blockIdx.x; i < count; i += gridDim.x) {
            const int4 item = hot_items[i];
            hv_tile_item<QUEUE, MODE>(item.x, item.y, item.z & 0xff, item.z >> 8, item.w, QUEUE ? 1 : ntiles, CV_TILE_ITEM_ARGS, tab);
            __syncthreads();          // (the next item reuses the workgroup's LDS)
        }
        return;
    }
    int y, tile, part, nparts, slot0, slot_stride;
    if (QUEUE) {
        if ((int)blockIdx.x >= list_ctl[2]) return;
        const int4 item = items[blockIdx.x];
        y = item.x; tile = item.y; part = item.z & 0xff; nparts = item.z >> 8; slot0 = item.w; slot_stride = 1;
    } else {
        tile = blockIdx.x % ntiles;
        const int4 qi = q_info[blockIdx.x / ntiles];     // (plane, part) slot
        if (qi.z < 0) return;
        y = qi.x; part = qi.y; nparts = qi.z;
        slot0 = qi.w * ntiles + tile; slot_stride = ntiles;
    }
    hv_tile_item<QUEUE, MODE>(y, tile, part, nparts, slot0, slot_stride, CV_TILE_ITEM_ARGS, tab);
#undef CV_TILE_ITEM_ARGS
}
template <bool QUEUE, int MODE>
__global__ __launch_bounds__(TW * 64) void hv_fwd_tiles(
    int R, float res, F3 corner, I3 dims, const float2* __restrict__ tab,
    const int* __restrict__ ystart, const int4* __restrict__ items, const float* __restrict__ rec,
    int64_t rec_stride, int tiles_x, int tiles_z, unsigned long long* __restrict__ partials,
    int* __restrict__ arrivals, float* __restrict__ g_obj, float* __restrict__ g_rot,
    float* __restrict__ g_scale, const int* __restrict__ list_ctl, const int* __restrict__ list_start, const int* __restrict__ list_cnt,
    const int2* __restrict__ entries, int list_mode /* 1: stream the bins, 2: work lists */,
    const int4* __restrict__ q_info, CatStride ks, int4* __restrict__ hot, float thresh, int4* __restrict__ hot_items) {
    ystart = cat_ws(ystart, ks.ws); items = cat_ws(items, ks.ws); rec = cat_ws(rec, ks.ws);
    partials = cat_ws(partials, ks.ws); arrivals = cat_ws(arrivals, ks.ws); list_ctl = cat_ws(list_ctl, ks.ws);
    list_start = cat_ws(list_start, ks.ws); list_cnt = cat_ws(list_cnt, ks.ws); entries = cat_ws(entries, ks.ws);
    q_info = cat_ws(q_info, ks.ws);
    g_obj = cat_el(g_obj, ks.cells); g_rot = cat_el(g_rot, 2 * ks.cells); g_scale = cat_el(g_scale, 3 * ks.cells);
    if (MODE != VOTE_FULL) { hot = cat_ws(hot, ks.ws); hot_items = cat_ws(hot_items, ks.ws); }
    fwd_tiles_body<QUEUE, MODE>(R, res, corner, dims, tab, ystart, items, rec, rec_stride, tiles_x, tiles_z, partials, arrivals, g_obj,
                                g_rot, g_scale, list_ctl, list_start, list_cnt, entries, list_mode, q_info, hot, thresh, hot_items);
}

// ---------------------------------------------------------------------------
// (Round 3, measured and removed - git 5179aa0 holds the code: a ROLLING tile kernel, one workgroup per tile and RANGE of
// planes with two planes in LDS, every vote expanded once and accumulated into both of its planes, plane s stored after
// bin s.  Exact (all vote / decode / concurrency tests), half the cull and expansion work - and 0.56-0.85 ms against
// 0.37-0.44 ms for hv_fwd_tiles in every tile width / waves / range-count configuration, fastest with the MOST ranges
// (profiles/r3/vote_roll_sweep.txt): the op is bound by how many latency chains run side by side, not by the work in
// them; a serial bin loop per workgroup takes parallelism away.)
// ---------------------------------------------------------------------------
// ---------------------------------------------------------------------------
// backward (hv_cuda_kernel.cu:168-261): one wave per point, lanes over rotations,
// butterfly reduction (deterministic; no atomics, like the reference).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hv_bwd(
    const float* __restrict__ grad, const float* __restrict__ pts, const float* __restrict__ xyz,
    const float* __restrict__ scl, const float* __restrict__ obj, int64_t n, int R, float res,
    F3 corner, I3 dims, const float2* __restrict__ tab, float* __restrict__ d_xyz,
    float* __restrict__ d_scl, float* __restrict__ d_obj) {
    const int lane = threadIdx.x & 63;
    const int64_t c = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (c >= n) return;
    const int Y = dims.y, Z = dims.z;
    const float s0 = scl[c * 3 + 0], s1 = scl[c * 3 + 1], s2 = scl[c * 3 + 2];
    const float x0 = xyz[c * 3 + 0], x1 = xyz[c * 3 + 1], x2 = xyz[c * 3 + 2];
    const float cx = x0 * s0, cy = x1 * s1, cz = x2 * s2;
    const float px = pts[c * 3 + 0], py = pts[c * 3 + 1], pz = pts[c * 3 + 2];
    const float ob = obj[c];
    float a_obj = 0, a_x0 = 0, a_x1 = 0, a_x2 = 0, a_s0 = 0, a_s1 = 0, a_s2 = 0;
    for (int i = lane; i < R; i += 64) {
        const float2 cs = tab[i];
        const float ox = (-cs.x) * cx + cs.y * cz;
        const float oy = -cy;
        const float oz = (-cs.y) * cx - cs.x * cz;
        const float gx = grid_pos(px, ox, corner.x, res);
        const float gy = grid_pos(py, oy, corner.y, res);
        const float gz = grid_pos(pz, oz, corner.z, res);
        if (gx < 0 || gy < 0 || gz < 0 || gx >= (float)(dims.x - 1) || gy >= (float)(dims.y - 1) ||
            gz >= (float)(dims.z - 1))
            continue;
        const int fx = (int)gx, fy = (int)gy, fz = (int)gz;
        const float rx = gx - floorf(gx), ry = gy - floorf(gy), rz = gz - floorf(gz);
        const float w0x = 1.f - rx, w0y = 1.f - ry, w0z = 1.f - rz, w1x = rx, w1y = ry, w1z = rz;
        const int64_t b = ((int64_t)fx * Y + fy) * Z + fz;
        const int64_t sx = (int64_t)Y * Z, sy = Z;
        const float lll = grad[b], llh = grad[b + 1], lhl = grad[b + sy], lhh = grad[b + sy + 1];
        const float hll = grad[b + sx], hlh = grad[b + sx + 1], hhl = grad[b + sx + sy],
                    hhh = grad[b + sx + sy + 1];
        float dob = lll * w0x * w0y * w0z;
        dob += llh * w0x * w0y * w1z;
        dob += lhl * w0x * w1y * w0z;
        dob += lhh * w0x * w1y * w1z;
        dob += hll * w1x * w0y * w0z;
        dob += hlh * w1x * w0y * w1z;
        dob += hhl * w1x * w1y * w0z;
        dob += hhh * w1x * w1y * w1z;
        a_obj += dob;
        float dx = -lll * w0y * w0z;
        dx = dx - llh * w0y * w1z; dx = dx - lhl * w1y * w0z; dx = dx - lhh * w1y * w1z;
        dx = dx + hll * w0y * w0z; dx = dx + hlh * w0y * w1z; dx = dx + hhl * w1y * w0z;
        dx = dx + hhh * w1y * w1z;
        float dy = -lll * w0x * w0z;
        dy = dy - llh * w0x * w1z; dy = dy + lhl * w0x * w0z; dy = dy + lhh * w0x * w1z;
        dy = dy - hll * w1x * w0z; dy = dy - hlh * w1x * w1z; dy = dy + hhl * w1x * w0z;
        dy = dy + hhh * w1x * w1z;
        float dz = -lll * w0x * w0y;
        dz = dz + llh * w0x * w0y; dz = dz - lhl * w0x * w1y; dz = dz + lhh * w0x * w1y;
        dz = dz - hll * w1x * w0y; dz = dz + hlh * w1x * w0y; dz = dz - hhl * w1x * w1y;
        dz = dz + hhh * w1x * w1y;
        dx *= ob; dy *= ob; dz *= ob;
        const float dcx = (-cs.x) * dx - cs.y * dz;
        const float dcy = -dy;
        const float dcz = cs.y * dx - cs.x * dz;
        a_x0 += dcx * s0; a_x1 += dcy * s1; a_x2 += dcz * s2;
        a_s0 += dcx * x0; a_s1 += dcy * x1; a_s2 += dcz * x2;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a_obj += __shfl_xor(a_obj, off);
        a_x0 += __shfl_xor(a_x0, off); a_x1 += __shfl_xor(a_x1, off); a_x2 += __shfl_xor(a_x2, off);
        a_s0 += __shfl_xor(a_s0, off); a_s1 += __shfl_xor(a_s1, off); a_s2 += __shfl_xor(a_s2, off);
    }
    if (lane == 0) {
        d_obj[c] = a_obj;
        d_xyz[c * 3 + 0] = a_x0; d_xyz[c * 3 + 1] = a_x1; d_xyz[c * 3 + 2] = a_x2;
        d_scl[c * 3 + 0] = a_s0; d_scl[c * 3 + 1] = a_s1; d_scl[c * 3 + 2] = a_s2;
    }
}

__global__ __launch_bounds__(256) void hv_count_votes(
    const float* __restrict__ pts, const float* __restrict__ xyz, const float* __restrict__ scl,
    int64_t n, int R, float res, F3 corner, I3 dims, const float2* __restrict__ tab,
    unsigned long long* __restrict__ count) {
    unsigned local = 0;
    for (int64_t t = blockIdx.x * 256ll + threadIdx.x; t < n * R; t += (int64_t)gridDim.x * 256) {
        const int64_t c = t / R;
        const int i = (int)(t - c * R);
        const float cx = xyz[c * 3 + 0] * scl[c * 3 + 0], cy = xyz[c * 3 + 1] * scl[c * 3 + 1],
                    cz = xyz[c * 3 + 2] * scl[c * 3 + 2];
        const float2 cs = tab[i];
        const float ox = (-cs.x) * cx + cs.y * cz, oy = -cy, oz = (-cs.y) * cx - cs.x * cz;
        const float gx = grid_pos(pts[c * 3 + 0], ox, corner.x, res);
        const float gy = grid_pos(pts[c * 3 + 1], oy, corner.y, res);
        const float gz = grid_pos(pts[c * 3 + 2], oz, corner.z, res);
        local += !(gx < 0 || gy < 0 || gz < 0 || gx >= (float)(dims.x - 1) ||
                   gy >= (float)(dims.y - 1) || gz >= (float)(dims.z - 1));
    }
    __shared__ unsigned s[256];
    s[threadIdx.x] = local;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) s[threadIdx.x] += s[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0 && s[0]) atomicAdd(count, (unsigned long long)s[0]);
}

// the zero-initialised words of K workspace carves in one launch (hipMemsetAsync covers one contiguous range: K of them
// would make the launch count grow with K)
__global__ __launch_bounds__(256) void hv_zero_cat(int* __restrict__ base, int64_t words, int64_t ks_ws) {
    base = cat_ws(base, ks_ws);
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) base[i] = 0;
}

int check_common(const void* a, const void* b, const void* c, int64_t n, float res, int num_rots,
                 const float* corner, const int* dims) {
    CV_REQUIRE(a && b && c && corner && dims, CV_EINVAL, "null pointer argument");
    CV_REQUIRE(n > 0, CV_EINVAL, "n must be positive (got %lld)", (long long)n);
    CV_REQUIRE(res > 0.f, CV_EINVAL, "res must be positive");
    CV_REQUIRE(num_rots > 0 && num_rots <= 4096, CV_EINVAL, "num_rots out of range (%d)", num_rots);
    CV_REQUIRE(dims[0] > 0 && dims[1] > 0 && dims[2] > 0, CV_EINVAL, "bad grid dims");
    CV_REQUIRE((int64_t)dims[0] * dims[1] * dims[2] < (1ll << 31), CV_EINVAL, "grid too large");
    CV_REQUIRE(n * (int64_t)num_rots < (1ll << 40), CV_EINVAL, "n*num_rots too large");
    return CV_OK;
}

// streaming launch (small grids): sum over planes of parts per tile: sum_y ceil(n2_y / PART_RECORDS) <= Y + 2n / PART_RECORDS
__host__ __device__ inline int64_t tiles_q_bound(int64_t n, int Y) { return (int64_t)Y + (2 * n + PART_RECORDS - 1) / PART_RECORDS; }
// the launch shape: work lists + work queue where a plane has many tiles (measured, bench vote stage: 300k-point scene,
// 200 tiles: 2.01 -> 1.32 ms; 80k scene, 66 tiles: 0.37 -> 0.40 ms - the weight pass and the queue build cost more than
// the tile kernel gains there; forced either way in flight: profiles/r3/vote_tile_sweep.txt, r5/knobs_in_flight.txt), the
// streaming launch below that.  16-wide tiles: an 80k-point grid has 66 tiles, a 300k-point grid 190.
constexpr int QUEUE_MIN_TILES = 128;
constexpr int PEAK_WGS = 512;        // workgroups of the VOTE_PEAKS launch (two per CU); each strides over the listed items
// work queue: partial-tile slots for the (plane, tile) pairs with more than one part (sum of arc lengths <= about
// 2 * n * num_rots counting both planes of a vote and the slack steps; twice that again as room) and items = one per
// (plane, tile) + the extra parts; hv_build_queue falls back to one part per tile if either is exceeded
__host__ __device__ inline int64_t queue_max_slots(int64_t n, int num_rots) { return 4 * n * (int64_t)num_rots / PART_VOTES + 256; }
__host__ __device__ inline int64_t queue_max_items(int64_t n, int num_rots, int64_t Y, int64_t ntiles) { return Y * ntiles + queue_max_slots(n, num_rots); }
// capacity of the work-list array: 40 entries per point on average (a ring of 1.5 m radius crosses ~20 tiles) and never
// more than every (point, tile) pair; beyond it the tile kernel streams the bins as before
__host__ __device__ inline int64_t list_capacity(int64_t n, int64_t ntiles) { return n * ntiles < 40 * n + 65536 ? n * ntiles : 40 * n + 65536; }

// The workspace of the tile algorithm, stated ONCE: the launch shape, the bounds derived from it and every array of one
// category's carve, in carve order, each aligned to 256 bytes.  The size query, the category stride, the CV_ENOMEM check, the
// zero fill and the launches all read this (base = nullptr: sizes only).  The workspace follows the launch shape actually
// chosen: the streaming launch (80k-point scenes) takes none of the list / queue arrays (zero-length carves, nothing of it
// reads them; they were > 60 MB of every stream's 100 MB vote scratch until round 4).
// Host and device: a scene kernel (below) restates its job's layout from (carve base, n, num_rots, dims) - a table of the
// pointers themselves, 21 per job and their bounds, would not fit the kernel arguments sixteen times.
struct TilesLayout {
    bool queue;                    // work queue + work lists (large grids) or the streaming launch
    int tiles_x, tiles_z, ntiles;
    int64_t max_q;                 // streaming launch: (plane, part) slots
    int64_t max_items, max_slots;  // work queue: items and partial-tile slots
    int64_t list_cap, max_chunks;  // work lists: entries; chunks of LIST_CHUNK_RECORDS records of one bin
    int* fy; float* rec;
    int* list_ctl; int* list_cnt; int* tile_w; int* ycount; int* arrivals;      // zeroed by one fill: see zero_from
    int* ystart; int* cursor; int* part_start; int4* q_info;
    unsigned long long* partials;
    int4* items; int* list_start; int* chunk_start; int* bin_of_chunk; int* chunk_off; int2* entries;
    int4* hot_items;               // peak mode: the work items of the (plane, tile) pairs with a box, appended by VOTE_OBJ
    int4* hot;                     // peak mode: the HotBox of every (plane, tile), written by VOTE_OBJ and read by VOTE_PEAKS
    int* zero_from;                // list_ctl (queue; list_cnt is zeroed with the rest: the count pass adds to it) or ycount
    size_t zero_bytes;             // ... up to the end of arrivals (the streaming launch only needs ycount and arrivals zeroed)
    size_t bytes;                  // end of the last array, rounded up to 256: one category's workspace and the category stride
};
__host__ __device__ inline TilesLayout tiles_layout(int64_t n, int num_rots, const int* dims, void* base) {
    TilesLayout L{};
    const size_t Y = (size_t)dims[1];
    L.tiles_x = (dims[0] + TX - 1) / TX;
    L.tiles_z = (dims[2] + TZ - 1) / TZ;
    const int64_t ntiles = (int64_t)L.tiles_x * L.tiles_z;
    L.ntiles = (int)ntiles;
    L.max_q = tiles_q_bound(n, (int)Y);
    L.max_slots = queue_max_slots(n, num_rots);
    L.max_items = queue_max_items(n, num_rots, (int64_t)Y, ntiles);
    L.list_cap = list_capacity(n, ntiles);
    L.max_chunks = (int64_t)Y + (n + LIST_CHUNK_RECORDS - 1) / LIST_CHUNK_RECORDS;
    L.queue = ntiles >= QUEUE_MIN_TILES && ntiles <= LIST_MAX_TILES && L.list_cap < (1ll << 31) && L.max_items < (1ll << 31);
    const size_t q = L.queue ? 1 : 0, planes = Y * (size_t)ntiles;
    size_t off = 0;
    auto take = [&](auto*& p, size_t count) {      // the array's first byte
        off = cv_align_up(off, 256);
        const size_t at = off;
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(reinterpret_cast<uintptr_t>(base) + at);
        off += count * sizeof(*p);
        return at;
    };
    take(L.fy, (size_t)n);
    take(L.rec, (size_t)n * REC_F);
    const size_t ctl_at = take(L.list_ctl, 64);
    take(L.list_cnt, q * planes);
    take(L.tile_w, q * planes);
    const size_t ycount_at = take(L.ycount, Y);
    // (+ 1: arrivals[planes] is the length of hot_items - VOTE_OBJ counts it up from the zero the per-call fill below leaves there)
    take(L.arrivals, planes + 1);
    L.zero_from = L.queue ? L.list_ctl : L.ycount;
    L.zero_bytes = off - (L.queue ? ctl_at : ycount_at);
    take(L.ystart, Y + 1);
    take(L.cursor, Y);
    take(L.part_start, Y + 1);
    take(L.q_info, (size_t)L.max_q);
    take(L.partials, (size_t)(L.queue ? L.max_slots : L.max_q * ntiles) * 6 * TCELLS);
    take(L.items, q * (size_t)L.max_items);
    take(L.list_start, q * planes);
    take(L.chunk_start, Y + 1);
    take(L.bin_of_chunk, (size_t)L.max_chunks);
    take(L.chunk_off, q * (size_t)L.max_chunks * (size_t)ntiles);
    take(L.entries, q * (size_t)L.list_cap);
    take(L.hot, planes);
    take(L.hot_items, (size_t)(L.queue ? L.max_items : L.max_q * ntiles));
    L.bytes = cv_align_up(off, 256);
    return L;
}

bool algo_ok(int algo) { return algo >= 0 && algo <= 2; }      // include/cv_hip.h: 0 auto, 1 direct, 2 tiles
int pick_algo(int algo, int64_t n, int num_rots) {
    if (algo == 1 || algo == 2) return algo;
    if (num_rots <= MAX_R_TILES && n < (1ll << 31)) return 2;
    return 1;
}

// ---- Scene axis (cv_hv_forward_scenes_f32): B votes that share nothing but res, num_rots and the rotation table.  Job b votes
// the rows [row0, row0 + n) of the shared point / prediction arrays onto its own corner and shape, into its own grid triple, on
// its own workspace carve `ws_off` bytes into the call's workspace.  The job table travels by value in the kernel arguments,
// launch dimension y is the job (as hv_decode.hip's scene axis), and a workgroup restates the TilesLayout of its job - every
// counter, record, list, partial slot, arrival word and hot-item list is the job's own, and so are Y, the tile counts, max_q and
// the LDS-histogram choice.  Launch extents are the maximum over the jobs: a workgroup beyond its own job's extent returns as
// a whole before its first barrier.  The bodies are the category kernels' bodies: a job's grids are the single call's bits.
struct VoteSceneJob {
    float* g_obj; float* g_rot; float* g_scale;
    int64_t ws_off, row0;
    int n;
    I3 dims;
    F3 corner;
};
struct VoteScenes {
    VoteSceneJob j[CV_MAX_SCENES];
    char* ws;
    int R;
};
static_assert(sizeof(VoteScenes) + 128 <= 4096, "the job table and the other arguments of a scene kernel are kernel arguments");

__device__ __forceinline__ TilesLayout scene_layout(const VoteScenes& js, const VoteSceneJob& j) {
    const int d[3] = {j.dims.x, j.dims.y, j.dims.z};
    return tiles_layout(j.n, js.R, d, js.ws + j.ws_off);
}

// every word the kernels of a job rely on being zero, for all jobs in one launch
__global__ __launch_bounds__(256) void hv_zero_scenes(VoteScenes js) {
    const VoteSceneJob& j = js.j[blockIdx.y];
    const TilesLayout L = scene_layout(js, j);
    const int64_t words = (int64_t)(L.zero_bytes / 4);
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) L.zero_from[i] = 0;
}
__global__ __launch_bounds__(PREP_THREADS) void hv_prep_count_scenes(VoteScenes js, const float* __restrict__ pts,
                                                                     const float* __restrict__ xyz,
                                                                     const float* __restrict__ scl, float res) {
    const VoteSceneJob& j = js.j[blockIdx.y];
    if ((int64_t)blockIdx.x * PREP_THREADS >= j.n) return;
    const TilesLayout L = scene_layout(js, j);
    prep_count_body(pts + j.row0 * 3, xyz + j.row0 * 3, scl + j.row0 * 3, j.n, res, j.corner.y, j.dims.y, L.fy, L.ycount);
}
__global__ __launch_bounds__(256) void hv_prep_scan_scenes(VoteScenes js, int part_records) {
    const VoteSceneJob& j = js.j[blockIdx.y];
    const TilesLayout L = scene_layout(js, j);
    prep_scan_body(L.ycount, j.dims.y, L.ystart, L.cursor, L.part_start, L.q_info, (int)L.max_q, L.chunk_start, L.bin_of_chunk,
                   part_records);
}
__global__ __launch_bounds__(PREP_THREADS) void hv_prep_scatter_scenes(VoteScenes js, const float* __restrict__ pts,
                                                                       const float* __restrict__ xyz,
                                                                       const float* __restrict__ scl,
                                                                       const float* __restrict__ obj, float res) {
    const VoteSceneJob& j = js.j[blockIdx.y];
    if ((int64_t)blockIdx.x * PREP_THREADS >= j.n) return;
    const TilesLayout L = scene_layout(js, j);
    prep_scatter_body(pts + j.row0 * 3, xyz + j.row0 * 3, scl + j.row0 * 3, obj + j.row0, L.fy, j.n, j.dims.y, res, j.corner,
                      L.cursor, L.rec, j.n);
}
// (the list and queue passes: jobs on the streaming side of QUEUE_MIN_TILES return at once)
template <bool FILL>
__global__ __launch_bounds__(1024) void hv_list_pass_scenes(VoteScenes js) {
    const VoteSceneJob& j = js.j[blockIdx.y];
    const TilesLayout L = scene_layout(js, j);
    if (!L.queue || (int64_t)blockIdx.x >= L.max_chunks) return;
    list_pass_body<FILL>(L.ystart, L.chunk_start, L.bin_of_chunk, j.dims.y, L.rec, j.n, js.R, L.tiles_x, L.tiles_z, L.list_ctl,
                         L.list_cnt, L.list_start, L.chunk_off, L.entries, L.tile_w, 1);
}
__global__ __launch_bounds__(1024) void hv_build_queue_scenes(VoteScenes js) {
    const VoteSceneJob& j = js.j[blockIdx.y];
    const TilesLayout L = scene_layout(js, j);
    if (!L.queue) return;
    build_queue_body(L.tile_w, j.dims.y, L.ntiles, (int)L.max_items, (int)L.max_slots, L.list_ctl, L.items);
}
__global__ __launch_bounds__(1024) void hv_list_scan_scenes(VoteScenes js) {
    const VoteSceneJob& j = js.j[blockIdx.y];
    const TilesLayout L = scene_layout(js, j);
    if (!L.queue) return;
    list_scan_body(L.list_cnt, j.dims.y, L.ntiles, L.list_cap, L.list_ctl, L.list_start);
}
// one launch per side of QUEUE_MIN_TILES that the batch has jobs on; each returns at once for the other side's jobs
template <bool QUEUE, int MODE>
__global__ __launch_bounds__(TW * 64) void hv_fwd_tiles_scenes(VoteScenes js, float res, const float2* __restrict__ tab,
                                                               float thresh) {
    const VoteSceneJob& j = js.j[blockIdx.y];
    const TilesLayout L = scene_layout(js, j);
    if (L.queue != QUEUE) return;
    if ((int64_t)blockIdx.x >= (QUEUE ? L.max_items : L.max_q * L.ntiles)) return;
    fwd_tiles_body<QUEUE, MODE>(js.R, res, j.corner, j.dims, tab, L.ystart, L.items, L.rec, j.n, L.tiles_x, L.tiles_z, L.partials,
                                L.arrivals, j.g_obj, j.g_rot, j.g_scale, L.list_ctl, L.list_start, L.list_cnt, L.entries,
                                QUEUE ? 2 : 1, L.q_info, L.hot, thresh, L.hot_items);
}

}  // namespace

extern "C" {

size_t cv_hv_minmax_workspace_bytes(void) { return 256 + sizeof(float) * 6 * (MM_BLOCKS + 1) + 256; }

int cv_hv_minmax_f32(const float* d_points, int64_t n, float* h_min3, float* h_max3, void* d_ws,
                     size_t ws_bytes, void* stream) {
    CV_REQUIRE(h_min3 && h_max3, CV_EINVAL, "null pointer argument");
    float h[6];
    const int rc = cv_hv_minmax_async_ex(d_points, n, h, d_ws, ws_bytes, nullptr, nullptr, stream);
    if (rc) return rc;
    CV_HIP_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    for (int k = 0; k < 3; ++k) { h_min3[k] = h[k]; h_max3[k] = h[3 + k]; }
    return CV_OK;
}

// Same reduction without the host wait: h_minmax6 (PINNED host memory: min xyz, max xyz) is valid once the
// work enqueued on `stream` up to this call has completed (record an event after it).  Lets a pipeline start
// the bounds reduction of a scene before its network forward instead of stalling in front of the vote.
int cv_hv_minmax_async_f32(const float* d_points, int64_t n, float* h_minmax6, void* d_ws, size_t ws_bytes,
                           void* stream) {
    return cv_hv_minmax_async_ex(d_points, n, h_minmax6, d_ws, ws_bytes, nullptr, nullptr, stream);
}

}  // extern "C"

// (C++ linkage, cv_common.h) d_zero_word / d_fill7f: one word set to 0 and eight words set to 0x7f7f7f7f by the final launch
int cv_hv_minmax_async_ex(const float* d_points, int64_t n, float* h_minmax6, void* d_ws, size_t ws_bytes, int32_t* d_zero_word,
                          int32_t* d_fill7f, void* stream) {
    CV_REQUIRE(d_points && h_minmax6 && d_ws, CV_EINVAL, "null pointer argument");
    CV_REQUIRE(n > 0, CV_EINVAL, "n must be positive (got %lld)", (long long)n);
    CV_REQUIRE(ws_bytes >= cv_hv_minmax_workspace_bytes(), CV_ENOMEM, "workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CvCarver cv(d_ws);
    float* part = cv.take<float>(6 * MM_BLOCKS);
    float* out = cv.take<float>(6);
    const int blocks = (int)std::min<int64_t>(MM_BLOCKS, (n + 255) / 256);
    minmax_partial<<<blocks, 256, 0, st>>>(d_points, n, part);
    CV_LAUNCH_CHECK();
    minmax_final<<<1, 256, 0, st>>>(part, blocks, out, d_zero_word, d_fill7f);
    CV_LAUNCH_CHECK();
    CV_HIP_CHECK(hipMemcpyAsync(h_minmax6, out, 6 * sizeof(float), hipMemcpyDeviceToHost, st));
    return CV_OK;
}

// (C++ linkage, cv_common.h) the scene axis of the reduction above: one launch, one copy
int cv_hv_scene_bounds_async_ex(const int32_t* d_coords4, const float* d_points, int64_t n, int num_scenes, int32_t* h_out,
                                void* d_ws, size_t ws_bytes, int32_t* d_zero_word, int32_t* d_fill7f, void* stream) {
    CV_REQUIRE(d_coords4 && d_points && h_out && d_ws, CV_EINVAL, "null pointer argument");
    CV_REQUIRE(n > 0 && n < (1ll << 31), CV_EINVAL, "n out of range (got %lld)", (long long)n);
    CV_REQUIRE(num_scenes >= 1 && num_scenes <= CV_MAX_SCENES, CV_EINVAL, "num_scenes out of range (%d, 1..%d)", num_scenes,
               CV_MAX_SCENES);
    static_assert(sizeof(int32_t) * SB_WORDS * CV_MAX_SCENES <= sizeof(float) * 6 * MM_BLOCKS, "fits the minmax workspace");
    CV_REQUIRE(ws_bytes >= cv_hv_minmax_workspace_bytes(), CV_ENOMEM, "workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t* out = static_cast<int32_t*>(d_ws);
    scene_bounds<<<num_scenes, SB_T, 0, st>>>(d_coords4, d_points, n, num_scenes, out, d_zero_word, d_fill7f);
    CV_LAUNCH_CHECK();
    CV_HIP_CHECK(hipMemcpyAsync(h_out, out, sizeof(int32_t) * SB_WORDS * num_scenes, hipMemcpyDeviceToHost, st));
    return CV_OK;
}

extern "C" {

int cv_hv_grid_dims_f32(const float h_min3[3], const float h_max3[3], float res, int dims_out[3]) {
    CV_REQUIRE(h_min3 && h_max3 && dims_out, CV_EINVAL, "null pointer argument");
    CV_REQUIRE(res > 0.f, CV_EINVAL, "res must be positive");
    for (int k = 0; k < 3; ++k) {
        volatile float d = h_max3[k] - h_min3[k];   // hv_cuda_kernel.cu:131 (fp32 tensor ops)
        volatile float q = d / res;
        dims_out[k] = (int)q + 1;                   // :132 .item().to<int>() + 1
    }
    return CV_OK;
}

size_t cv_hv_forward_workspace_bytes(int64_t n, int num_rots, const int dims[3], int algo) {
    if (!dims || n <= 0 || !algo_ok(algo)) return 0;
    if (pick_algo(algo, n, num_rots) == 1) return 256;
    return tiles_layout(n, num_rots, dims, nullptr).bytes;
}

// cv_hv_set_kernel_events: the calling thread's next cv_hv_forward_f32 calls record these events directly before and
// after the accumulation (hv_fwd_tiles; peak mode: in front of the first and behind the second of its two launches), on the
// stream of the call
static thread_local hipEvent_t t_ev_start = nullptr, t_ev_stop = nullptr;

// records of a plane's two y-bins one workgroup of a hot (tile, plane) takes in the streaming launch: PART_RECORDS (the workspace
// bound assumes at least that many) or more - with several scenes in flight fewer, longer parts pay (less merge traffic, the other
// scenes fill the chip): profiles/r5/vote_parts.txt
static std::atomic<long long> g_part_records{getenv("CV_HV_PART_RECORDS") ? std::max<long long>(PART_RECORDS, atoll(getenv("CV_HV_PART_RECORDS")))
                                                                          : (long long)PART_RECORDS};

static thread_local long long t_part_records = 0;     // cv_hv_set_part_records_thread: this thread's launches (0 = process-wide)

int cv_hv_set_part_records(int records) {
    const long long v = records <= 0 ? (long long)PART_RECORDS : std::max<long long>(PART_RECORDS, records);
    return (int)g_part_records.exchange(v, std::memory_order_relaxed);
}

int cv_hv_set_part_records_thread(int records) {
    const int before = (int)t_part_records;
    t_part_records = records <= 0 ? 0 : std::max<long long>(PART_RECORDS, records);
    return before;
}

int cv_hv_set_kernel_events(void* ev_start, void* ev_stop) {
    t_ev_start = static_cast<hipEvent_t>(ev_start);
    t_ev_stop = static_cast<hipEvent_t>(ev_stop);
    return CV_OK;
}

// (a multiple of 256: it is also the byte distance of two categories' carves; the last category needs only the single carve)
size_t cv_hv_forward_cat_workspace_bytes(int64_t n, int num_rots, const int dims[3], int algo, int num_cats) {
    if (num_cats < 1 || num_cats > CV_MAX_CATEGORIES) return 0;
    return (size_t)num_cats * cv_hv_forward_workspace_bytes(n, num_rots, dims, algo);
}

// K categories over the same scan points and grid (K = 1: cv_hv_forward_f32).  Category k reads d_xyz / d_scale + 3 n k,
// d_obj + n k and writes the grids + (1, 2, 3) * cells * k; its workspace carve starts TilesLayout::bytes * k bytes into d_ws.
// peaks (tiles algorithm only; the direct one writes full grids either way): VOTE_OBJ then VOTE_PEAKS back to back instead of
// VOTE_FULL - the same d_grid_obj, d_grid_rot / d_grid_scale written at the cells with d_grid_obj >= thresh only.
static int hv_forward_cats(const float* d_points, const float* d_xyz, const float* d_scale, const float* d_obj, int64_t n,
                           float res, int num_rots, const float h_corner3[3], const int dims[3], float* d_grid_obj,
                           float* d_grid_rot, float* d_grid_scale, void* d_ws, size_t ws_bytes, int algo, int K,
                           hipStream_t st, bool peaks = false, float thresh = 0.f) {
    int rc = CV_OK;
    const float2* tab = nullptr;
    rc = get_rot_table(num_rots, &tab);
    if (rc) return rc;
    const F3 corner{h_corner3[0], h_corner3[1], h_corner3[2]};
    const I3 d3{dims[0], dims[1], dims[2]};
    const int64_t cells = (int64_t)dims[0] * dims[1] * dims[2];
    const int a = pick_algo(algo, n, num_rots);
    if (a == 2) CV_REQUIRE(num_rots <= MAX_R_TILES, CV_EINVAL, "tiles algorithm needs num_rots <= %d", MAX_R_TILES);
    if (a == 1) {
        // (not the hot path: the categories one after another)
        for (int k = 0; k < K; ++k) {
            float* g_obj = d_grid_obj + (int64_t)k * cells;
            float* g_rot = d_grid_rot + (int64_t)k * cells * 2;
            float* g_scale = d_grid_scale + (int64_t)k * cells * 3;
            CV_HIP_CHECK(hipMemsetAsync(g_obj, 0, sizeof(float) * cells, st));
            CV_HIP_CHECK(hipMemsetAsync(g_rot, 0, sizeof(float) * cells * 2, st));
            CV_HIP_CHECK(hipMemsetAsync(g_scale, 0, sizeof(float) * cells * 3, st));
            const int64_t total = n * num_rots;
            hv_fwd_direct<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(
                d_points, d_xyz + (int64_t)k * n * 3, d_scale + (int64_t)k * n * 3, d_obj + (int64_t)k * n, n, num_rots, res,
                corner, d3, tab, g_obj, g_rot, g_scale);
            CV_LAUNCH_CHECK();
            hv_normalise<<<(unsigned)((cells + 255) / 256), 256, 0, st>>>(g_obj, g_rot, g_scale, cells);
            CV_LAUNCH_CHECK();
        }
        return CV_OK;
    }
    const int Y = dims[1];
    const TilesLayout L = tiles_layout(n, num_rots, dims, d_ws);
    CV_REQUIRE(d_ws && ws_bytes >= (size_t)K * L.bytes, CV_ENOMEM, "workspace too small for the tiles algorithm");
    const CatStride ks{K > 1 ? (int64_t)L.bytes : 0, n, cells};
    const int tiles_x = L.tiles_x, tiles_z = L.tiles_z, ntiles = L.ntiles;
    const bool queue = L.queue;
    const int list_mode = queue ? 2 : 1;
    if (K == 1) CV_HIP_CHECK(hipMemsetAsync(L.zero_from, 0, L.zero_bytes, st));
    else {
        hv_zero_cat<<<dim3((unsigned)std::min<size_t>((L.zero_bytes / 4 + 255) / 256, 1024), K), 256, 0, st>>>(L.zero_from,
                                                                                                          L.zero_bytes / 4, ks.ws);
        CV_LAUNCH_CHECK();
    }
    const unsigned prep_wgs = (unsigned)((n + PREP_THREADS - 1) / PREP_THREADS);
    hv_prep_count<<<dim3(prep_wgs, K), PREP_THREADS, 0, st>>>(d_points, d_xyz, d_scale, n, res, corner.y, Y, L.fy, L.ycount, ks);
    CV_LAUNCH_CHECK();
    hv_prep_scan<<<dim3(1, K), 256, 0, st>>>(L.ycount, Y, L.ystart, L.cursor, L.part_start, L.q_info, (int)L.max_q, L.chunk_start,
                                             L.bin_of_chunk,
                                             (int)(t_part_records > 0 ? t_part_records : g_part_records.load(std::memory_order_relaxed)),
                                             ks.ws);
    CV_LAUNCH_CHECK();
    hv_prep_scatter<<<dim3(prep_wgs, K), PREP_THREADS, 0, st>>>(d_points, d_xyz, d_scale, d_obj, L.fy, n, Y, res, corner, L.cursor,
                                                                 L.rec, n, ks);
    CV_LAUNCH_CHECK();
    if (queue) {
        hv_list_pass<false><<<dim3((unsigned)L.max_chunks, K), 1024, 0, st>>>(L.ystart, L.chunk_start, L.bin_of_chunk, Y, L.rec, n,
                                                                               num_rots, tiles_x, tiles_z, L.list_ctl, L.list_cnt,
                                                                               L.list_start, L.chunk_off, L.entries, L.tile_w, 1, ks.ws);
        CV_LAUNCH_CHECK();
        hv_build_queue<<<dim3(1, K), 1024, 0, st>>>(L.tile_w, Y, ntiles, (int)L.max_items, (int)L.max_slots, L.list_ctl, L.items,
                                                    ks.ws);
        CV_LAUNCH_CHECK();
        hv_list_scan<<<dim3(1, K), 1024, 0, st>>>(L.list_cnt, Y, ntiles, L.list_cap, L.list_ctl, L.list_start, ks.ws);
        CV_LAUNCH_CHECK();
        hv_list_pass<true><<<dim3((unsigned)L.max_chunks, K), 1024, 0, st>>>(L.ystart, L.chunk_start, L.bin_of_chunk, Y, L.rec, n,
                                                                              num_rots, tiles_x, tiles_z, L.list_ctl, L.list_cnt,
                                                                              L.list_start, L.chunk_off, L.entries, L.tile_w, 1, ks.ws);
        CV_LAUNCH_CHECK();
    }
    const int64_t wgs = queue ? L.max_items : L.max_q * ntiles;
    CV_REQUIRE(wgs < (1ll << 31), CV_EINVAL, "grid too large");
#define CV_TILES_ARGS num_rots, res, corner, d3, tab, L.ystart, L.items, L.rec, n, tiles_x, tiles_z, L.partials, L.arrivals, d_grid_obj, \
                      d_grid_rot, d_grid_scale, L.list_ctl, L.list_start, L.list_cnt, L.entries, list_mode, L.q_info, ks, L.hot, thresh, L.hot_items
#define CV_TILES_LAUNCH(MODE, WGS)                                                                           \
    do {                                                                                                      \
        if (queue) hv_fwd_tiles<true, MODE><<<dim3((unsigned)(WGS), K), TW * 64, 0, st>>>(CV_TILES_ARGS);     \
        else hv_fwd_tiles<false, MODE><<<dim3((unsigned)(WGS), K), TW * 64, 0, st>>>(CV_TILES_ARGS);          \
    } while (0)
    if (t_ev_start) CV_HIP_CHECK(hipEventRecord(t_ev_start, st));
    if (peaks) {
        // (the hot boxes stay on the device; VOTE_OBJ leaves the arrival counters at zero for VOTE_PEAKS)
        CV_TILES_LAUNCH(VOTE_OBJ, wgs);
        CV_LAUNCH_CHECK();
        CV_TILES_LAUNCH(VOTE_PEAKS, std::min<int64_t>(wgs, PEAK_WGS));
    } else {
        CV_TILES_LAUNCH(VOTE_FULL, wgs);
    }
    if (t_ev_stop) CV_HIP_CHECK(hipEventRecord(t_ev_stop, st));
#undef CV_TILES_LAUNCH
#undef CV_TILES_ARGS
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_hv_forward_f32(const float* d_points, const float* d_xyz, const float* d_scale,
                      const float* d_obj, int64_t n, float res, int num_rots,
                      const float h_corner3[3], const int dims[3], float* d_grid_obj,
                      float* d_grid_rot, float* d_grid_scale, void* d_ws, size_t ws_bytes, int algo,
                      void* stream) {
    CV_REQUIRE(algo_ok(algo), CV_EINVAL, "algo out of range (%d: 0 auto, 1 direct, 2 tiles)", algo);
    int rc = check_common(d_points, d_xyz, d_scale, n, res, num_rots, h_corner3, dims);
    if (rc) return rc;
    CV_REQUIRE(d_obj && d_grid_obj && d_grid_rot && d_grid_scale, CV_EINVAL, "null pointer argument");
    return hv_forward_cats(d_points, d_xyz, d_scale, d_obj, n, res, num_rots, h_corner3, dims, d_grid_obj, d_grid_rot, d_grid_scale,
                           d_ws, ws_bytes, algo, 1, static_cast<hipStream_t>(stream));
}

int cv_hv_forward_cat_f32(const float* d_points, const float* d_xyz, const float* d_scale, const float* d_obj, int64_t n,
                          float res, int num_rots, const float h_corner3[3], const int dims[3], int num_cats, float* d_grid_obj,
                          float* d_grid_rot, float* d_grid_scale, void* d_ws, size_t ws_bytes, int algo, void* stream) {
    CV_REQUIRE(num_cats >= 1 && num_cats <= CV_MAX_CATEGORIES, CV_EINVAL, "num_cats out of range (%d, 1..%d)", num_cats,
               CV_MAX_CATEGORIES);
    CV_REQUIRE(algo_ok(algo), CV_EINVAL, "algo out of range (%d: 0 auto, 1 direct, 2 tiles)", algo);
    int rc = check_common(d_points, d_xyz, d_scale, n, res, num_rots, h_corner3, dims);
    if (rc) return rc;
    CV_REQUIRE(d_obj && d_grid_obj && d_grid_rot && d_grid_scale, CV_EINVAL, "null pointer argument");
    return hv_forward_cats(d_points, d_xyz, d_scale, d_obj, n, res, num_rots, h_corner3, dims, d_grid_obj, d_grid_rot, d_grid_scale,
                           d_ws, ws_bytes, algo, num_cats, static_cast<hipStream_t>(stream));
}

int cv_hv_forward_peaks_f32(const float* d_points, const float* d_xyz, const float* d_scale, const float* d_obj, int64_t n,
                            float res, int num_rots, const float h_corner3[3], const int dims[3], float* d_grid_obj,
                            float* d_grid_rot, float* d_grid_scale, void* d_ws, size_t ws_bytes, int algo, float thresh,
                            void* stream) {
    CV_REQUIRE(algo_ok(algo), CV_EINVAL, "algo out of range (%d: 0 auto, 1 direct, 2 tiles)", algo);
    CV_REQUIRE(thresh == thresh, CV_EINVAL, "thresh is not a number");
    int rc = check_common(d_points, d_xyz, d_scale, n, res, num_rots, h_corner3, dims);
    if (rc) return rc;
    CV_REQUIRE(d_obj && d_grid_obj && d_grid_rot && d_grid_scale, CV_EINVAL, "null pointer argument");
    return hv_forward_cats(d_points, d_xyz, d_scale, d_obj, n, res, num_rots, h_corner3, dims, d_grid_obj, d_grid_rot, d_grid_scale,
                           d_ws, ws_bytes, algo, 1, static_cast<hipStream_t>(stream), true, thresh);
}

int cv_hv_forward_peaks_cat_f32(const float* d_points, const float* d_xyz, const float* d_scale, const float* d_obj, int64_t n,
                                float res, int num_rots, const float h_corner3[3], const int dims[3], int num_cats,
                                float* d_grid_obj, float* d_grid_rot, float* d_grid_scale, void* d_ws, size_t ws_bytes, int algo,
                                float thresh, void* stream) {
    CV_REQUIRE(num_cats >= 1 && num_cats <= CV_MAX_CATEGORIES, CV_EINVAL, "num_cats out of range (%d, 1..%d)", num_cats,
               CV_MAX_CATEGORIES);
    CV_REQUIRE(algo_ok(algo), CV_EINVAL, "algo out of range (%d: 0 auto, 1 direct, 2 tiles)", algo);
    CV_REQUIRE(thresh == thresh, CV_EINVAL, "thresh is not a number");
    int rc = check_common(d_points, d_xyz, d_scale, n, res, num_rots, h_corner3, dims);
    if (rc) return rc;
    CV_REQUIRE(d_obj && d_grid_obj && d_grid_rot && d_grid_scale, CV_EINVAL, "null pointer argument");
    return hv_forward_cats(d_points, d_xyz, d_scale, d_obj, n, res, num_rots, h_corner3, dims, d_grid_obj, d_grid_rot, d_grid_scale,
                           d_ws, ws_bytes, algo, num_cats, static_cast<hipStream_t>(stream), true, thresh);
}

// ---- scene axis -------------------------------------------------------------------------------------------------------------
// The workspace: the jobs' cv_hv_forward_workspace_bytes carved in job order (every one a multiple of 256), no table head.  The
// query, the CV_ENOMEM check and the carve offsets of the launches all read this; 0: a job the single query refuses.
static size_t scenes_workspace(const cv_decode_scene_job* jobs, int B, int num_rots, int algo, size_t* offs) {
    size_t total = 0;
    for (int b = 0; b < B; ++b) {
        const size_t one = jobs[b].n < (1ll << 31) ? cv_hv_forward_workspace_bytes(jobs[b].n, num_rots, jobs[b].dims, algo) : 0;
        if (one == 0) return 0;
        if (offs) offs[b] = total;
        total += cv_align_up(one, 256);
    }
    return total;
}

size_t cv_hv_forward_scenes_workspace_bytes(const cv_decode_scene_job* jobs, int num_scenes, int num_rots, int algo) {
    if (!jobs || num_scenes < 1 || num_scenes > CV_MAX_SCENES) return 0;
    return scenes_workspace(jobs, num_scenes, num_rots, algo, nullptr);
}

static int hv_forward_scenes(const cv_decode_scene_job* jobs, int B, const float* d_points, const float* d_xyz, const float* d_scale,
                             const float* d_obj, float res, int num_rots, void* d_ws, size_t ws_bytes, int algo, hipStream_t st,
                             bool peaks, float thresh) {
    // ---- refusals, all of them before the first device call
    CV_REQUIRE(B >= 1 && B <= CV_MAX_SCENES, CV_EINVAL, "num_scenes out of range (%d, 1..%d)", B, CV_MAX_SCENES);
    CV_REQUIRE(jobs && d_points && d_xyz && d_scale && d_obj, CV_EINVAL, "null pointer argument");
    CV_REQUIRE(algo_ok(algo), CV_EINVAL, "algo out of range (%d: 0 auto, 1 direct, 2 tiles)", algo);
    CV_REQUIRE(!peaks || thresh == thresh, CV_EINVAL, "thresh is not a number");
    CV_REQUIRE(res > 0.f, CV_EINVAL, "res must be positive");
    CV_REQUIRE(num_rots > 0 && num_rots <= 4096, CV_EINVAL, "num_rots out of range (%d)", num_rots);
    int a = 0;
    for (int b = 0; b < B; ++b) {
        const cv_decode_scene_job& j = jobs[b];
        CV_REQUIRE(j.d_grid_obj && j.d_grid_rot && j.d_grid_scale, CV_EINVAL, "scene %d: null grid pointer", b);
        CV_REQUIRE(j.n > 0 && j.n < (1ll << 31), CV_EINVAL, "scene %d: n out of range (got %lld)", b, (long long)j.n);
        CV_REQUIRE(j.row0 >= 0, CV_EINVAL, "scene %d: negative row0 (%lld)", b, (long long)j.row0);
        CV_REQUIRE(j.dims[0] > 0 && j.dims[1] > 0 && j.dims[2] > 0, CV_EINVAL, "scene %d: bad grid dims", b);
        CV_REQUIRE((int64_t)j.dims[0] * j.dims[1] * j.dims[2] < (1ll << 31), CV_EINVAL, "scene %d: grid too large", b);
        CV_REQUIRE(j.n * (int64_t)num_rots < (1ll << 40), CV_EINVAL, "scene %d: n*num_rots too large", b);
        // (pick_algo depends on num_rots and on n < 2^31 alone: one choice for the batch)
        a = pick_algo(algo, j.n, num_rots);
        if (a == 2) {
            CV_REQUIRE(num_rots <= MAX_R_TILES, CV_EINVAL, "tiles algorithm needs num_rots <= %d", MAX_R_TILES);
            const TilesLayout L = tiles_layout(j.n, num_rots, j.dims, nullptr);
            CV_REQUIRE((L.queue ? L.max_items : L.max_q * L.ntiles) < (1ll << 31), CV_EINVAL, "scene %d: grid too large", b);
        }
    }
    size_t offs[CV_MAX_SCENES];
    const size_t need = scenes_workspace(jobs, B, num_rots, algo, offs);
    CV_REQUIRE(need > 0 && d_ws && ws_bytes >= need, CV_ENOMEM, "workspace too small for %d scenes (needs %zu bytes)", B, need);

    // ---- one scene, or the direct kernel (not the hot path): the single call's launches, job after job
    if (B == 1 || a == 1) {
        for (int b = 0; b < B; ++b) {
            const cv_decode_scene_job& j = jobs[b];
            const size_t one = (b + 1 < B ? offs[b + 1] : need) - offs[b];
            const int rc = hv_forward_cats(d_points + j.row0 * 3, d_xyz + j.row0 * 3, d_scale + j.row0 * 3, d_obj + j.row0, j.n, res,
                                           num_rots, j.corner, j.dims, j.d_grid_obj, const_cast<float*>(j.d_grid_rot),
                                           const_cast<float*>(j.d_grid_scale), static_cast<char*>(d_ws) + offs[b], one, algo, 1, st,
                                           peaks, thresh);
            if (rc) return rc;
        }
        return CV_OK;
    }

    // ---- the tile algorithm over the scene axis
    const float2* tab = nullptr;
    const int rc = get_rot_table(num_rots, &tab);
    if (rc) return rc;
    VoteScenes js{};
    js.ws = static_cast<char*>(d_ws);
    js.R = num_rots;
    int64_t max_n = 0, zero_words = 0, max_chunks = 0, wgs[2] = {0, 0};       // launch extents: the maximum over the jobs
    for (int b = 0; b < B; ++b) {
        const cv_decode_scene_job& j = jobs[b];
        // (the one place the decode's job struct is written through: the vote fills the grids the decode reads)
        js.j[b] = VoteSceneJob{j.d_grid_obj, const_cast<float*>(j.d_grid_rot), const_cast<float*>(j.d_grid_scale), (int64_t)offs[b],
                               j.row0, (int)j.n, I3{j.dims[0], j.dims[1], j.dims[2]}, F3{j.corner[0], j.corner[1], j.corner[2]}};
        const TilesLayout L = tiles_layout(j.n, num_rots, j.dims, nullptr);
        max_n = std::max<int64_t>(max_n, j.n);
        zero_words = std::max<int64_t>(zero_words, (int64_t)(L.zero_bytes / 4));
        if (L.queue) max_chunks = std::max(max_chunks, L.max_chunks);
        wgs[L.queue] = std::max(wgs[L.queue], L.queue ? L.max_items : L.max_q * L.ntiles);
    }
    const unsigned prep_wgs = (unsigned)((max_n + PREP_THREADS - 1) / PREP_THREADS);
    const int part_records = (int)(t_part_records > 0 ? t_part_records : g_part_records.load(std::memory_order_relaxed));
    hv_zero_scenes<<<dim3((unsigned)std::min<int64_t>((zero_words + 255) / 256, 1024), B), 256, 0, st>>>(js);
    CV_LAUNCH_CHECK();
    hv_prep_count_scenes<<<dim3(prep_wgs, B), PREP_THREADS, 0, st>>>(js, d_points, d_xyz, d_scale, res);
    CV_LAUNCH_CHECK();
    hv_prep_scan_scenes<<<dim3(1, B), 256, 0, st>>>(js, part_records);
    CV_LAUNCH_CHECK();
    hv_prep_scatter_scenes<<<dim3(prep_wgs, B), PREP_THREADS, 0, st>>>(js, d_points, d_xyz, d_scale, d_obj, res);
    CV_LAUNCH_CHECK();
    if (wgs[1] > 0) {
        hv_list_pass_scenes<false><<<dim3((unsigned)max_chunks, B), 1024, 0, st>>>(js);
        CV_LAUNCH_CHECK();
        hv_build_queue_scenes<<<dim3(1, B), 1024, 0, st>>>(js);
        CV_LAUNCH_CHECK();
        hv_list_scan_scenes<<<dim3(1, B), 1024, 0, st>>>(js);
        CV_LAUNCH_CHECK();
        hv_list_pass_scenes<true><<<dim3((unsigned)max_chunks, B), 1024, 0, st>>>(js);
        CV_LAUNCH_CHECK();
    }
#define CV_SCENE_TILES(MODE, CAP)                                                                                              \
    do {                                                                                                                        \
        if (wgs[0] > 0) {                                                                                                       \
            hv_fwd_tiles_scenes<false, MODE><<<dim3((unsigned)std::min<int64_t>(wgs[0], CAP), B), TW * 64, 0, st>>>(js, res, tab, \
                                                                                                                    thresh);     \
            CV_LAUNCH_CHECK();                                                                                                  \
        }                                                                                                                       \
        if (wgs[1] > 0) {                                                                                                       \
            hv_fwd_tiles_scenes<true, MODE><<<dim3((unsigned)std::min<int64_t>(wgs[1], CAP), B), TW * 64, 0, st>>>(js, res, tab,  \
                                                                                                                   thresh);      \
            CV_LAUNCH_CHECK();                                                                                                  \
        }                                                                                                                       \
    } while (0)
    if (t_ev_start) CV_HIP_CHECK(hipEventRecord(t_ev_start, st));
    if (peaks) {
        CV_SCENE_TILES(VOTE_OBJ, (int64_t)1 << 31);
        CV_SCENE_TILES(VOTE_PEAKS, (int64_t)PEAK_WGS);
    } else {
        CV_SCENE_TILES(VOTE_FULL, (int64_t)1 << 31);
    }
    if (t_ev_stop) CV_HIP_CHECK(hipEventRecord(t_ev_stop, st));
#undef CV_SCENE_TILES
    return CV_OK;
}

int cv_hv_forward_scenes_f32(const cv_decode_scene_job* jobs, int num_scenes, const float* d_points, const float* d_xyz,
                             const float* d_scale, const float* d_obj, float res, int num_rots, void* d_ws, size_t ws_bytes,
                             int algo, void* stream) {
    return hv_forward_scenes(jobs, num_scenes, d_points, d_xyz, d_scale, d_obj, res, num_rots, d_ws, ws_bytes, algo,
                             static_cast<hipStream_t>(stream), false, 0.f);
}

int cv_hv_forward_peaks_scenes_f32(const cv_decode_scene_job* jobs, int num_scenes, const float* d_points, const float* d_xyz,
                                   const float* d_scale, const float* d_obj, float res, int num_rots, void* d_ws, size_t ws_bytes,
                                   int algo, float thresh, void* stream) {
    return hv_forward_scenes(jobs, num_scenes, d_points, d_xyz, d_scale, d_obj, res, num_rots, d_ws, ws_bytes, algo,
                             static_cast<hipStream_t>(stream), true, thresh);
}

int cv_hv_backward_f32(const float* d_grad_obj, const float* d_points, const float* d_xyz,
                       const float* d_scale, const float* d_obj, int64_t n, float res, int num_rots,
                       const float h_corner3[3], const int dims[3], float* d_dxyz, float* d_dscale,
                       float* d_dobj, void* stream) {
    int rc = check_common(d_points, d_xyz, d_scale, n, res, num_rots, h_corner3, dims);
    if (rc) return rc;
    CV_REQUIRE(d_grad_obj && d_obj && d_dxyz && d_dscale && d_dobj, CV_EINVAL, "null pointer argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float2* tab = nullptr;
    rc = get_rot_table(num_rots, &tab);
    if (rc) return rc;
    const F3 corner{h_corner3[0], h_corner3[1], h_corner3[2]};
    const I3 d3{dims[0], dims[1], dims[2]};
    hv_bwd<<<(unsigned)((n + 3) / 4), 256, 0, st>>>(d_grad_obj, d_points, d_xyz, d_scale, d_obj, n,
                                                   num_rots, res, corner, d3, tab, d_dxyz, d_dscale,
                                                   d_dobj);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_hv_count_votes_f32(const float* d_points, const float* d_xyz, const float* d_scale, int64_t n,
                          float res, int num_rots, const float h_corner3[3], const int dims[3],
                          int64_t* h_count, void* d_ws, size_t ws_bytes, void* stream) {
    int rc = check_common(d_points, d_xyz, d_scale, n, res, num_rots, h_corner3, dims);
    if (rc) return rc;
    CV_REQUIRE(h_count && d_ws && ws_bytes >= 256, CV_ENOMEM, "workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float2* tab = nullptr;
    rc = get_rot_table(num_rots, &tab);
    if (rc) return rc;
    unsigned long long* cnt = static_cast<unsigned long long*>(d_ws);
    CV_HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(*cnt), st));
    const F3 corner{h_corner3[0], h_corner3[1], h_corner3[2]};
    const I3 d3{dims[0], dims[1], dims[2]};
    const int64_t total = n * num_rots;
    hv_count_votes<<<(unsigned)std::min<int64_t>((total + 255) / 256, 2048), 256, 0, st>>>(
        d_points, d_xyz, d_scale, n, num_rots, res, corner, d3, tab, cnt);
    CV_LAUNCH_CHECK();
    unsigned long long h = 0;
    CV_HIP_CHECK(hipMemcpyAsync(&h, cnt, sizeof h, hipMemcpyDeviceToHost, st));
    CV_HIP_CHECK(hipStreamSynchronize(st));
    *h_count = (int64_t)h;
    return CV_OK;
}

}  // extern "C"
