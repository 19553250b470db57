// Detection decode for gfx950: greedy peak picking, grid suppression, LCC-aware
// back-projection check, class vote.
//
// Replaces the inline host loop eval_joint.py:195-263 (one full-grid argmax and >= 6
// device->host syncs per candidate) with three launches and ONE sync per scene:
//
//   dec_compact      cells with grid_obj >= thresh_high -> compact list (value, cell
//                    coordinates) PLUS the box geometry each cell would have as a candidate
//                    (rotation from the rot grid :213-214, scale :216): the double-precision
//                    atan2 / cos / sin of every listed cell are evaluated here, in parallel,
//                    instead of one at a time on the greedy loop's critical path.
//                    The loop stops when the maximum drops below thresh_high (:208-209)
//                    and only ever writes zeros, so cells below the threshold can never
//                    influence which candidates are examined.
//   dec_greedy_dispatch[_big]
//                    one workgroup walks the list (walk_lds, walk_global or walk_sorted, by the
//                    list length and the grid size): ONE pass and ONE barrier per candidate - the pass applies the suppression of the current candidate (the
//                    +-elimination cube :211 and the cells inside the oriented box :225-229,:243)
//                    to each entry and, for the survivors, accumulates the next argmax (ties ->
//                    lowest flat index, like torch.argmax).  The candidate sequence does not
//                    depend on the back-projection verdicts (the reference `continue`s after zeroing).
//   dec_backproject  all points x all candidates in parallel (:231-250): in-box test,
//                    counts, prob-weighted LCC error, max prob, class histogram; the last
//                    workgroup to finish turns the statistics into verdicts (:246-253), class
//                    mode (:255-256) and box corners (:258), one thread per candidate, and writes
//                    them straight into pinned host memory (no copy launch).
//
// fp32 conventions shared with oracle/decode_oracle.c (see its header): double-rounded
// atan2/cos/sin, k-ordered fmaf chain for the [.,3]@[3,3] products, x*(1/res) where
// torch divides by a python scalar, double accumulation of the masked mean.
// Compiled with -ffp-contract=off.
#include "cv_common.h"

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

namespace {

constexpr int NCLS = 64;   // class histogram bins (class ids must be in [0, 64))

struct Cand {
    long long idx;
    int c[3];
    int clo[3], chi[3];
    float cw[3];
    float cs, sn;
    float sc[3];
};

struct Stats {
    unsigned n_in, n_mask, pmax_bits;
    double err;
    unsigned hist[NCLS];
};
static_assert(offsetof(Stats, err) % 8 == 0, "64-bit atomic adds");
static_assert(sizeof(Stats) % 4 == 0, "a candidate's statistics are zeroed word by word");

struct Geo {
    int X, Y, Z;
    float corner[3];
    float res;
};

// compact list, structure of arrays over list positions
struct List {
    float* val;      // grid_obj value (zeroed when suppressed, global-array walk only)
    unsigned* xy;    // x | y << 16
    int* z;
    float* geo;      // [5][cap]: cos, sin, scale xyz of the box the cell would propose
    int64_t cap;
};

// flat cell index of a list entry (the walks order ties by it, like torch.argmax)
__device__ __forceinline__ int cell_id(const Geo& geo, unsigned xy, int z) {
    return ((int)(xy & 0xffffu) * geo.Y + (int)(xy >> 16)) * geo.Z + z;
}

// the counters block of a workspace carve: zeroed at the start of every call
constexpr int CTR_WORDS = 16;
constexpr int CTR_LIST_N = 0;     // list length (dec_compact)
constexpr int CTR_N_CAND = 4;     // candidate count, then the "truncated" flag (the walk)

// one category's workspace (WsLayout::at)
struct Ws {
    List L;
    unsigned* counters;
    Cand* cands;
    Stats* stats;
    __host__ __device__ unsigned* list_n() const { return counters + CTR_LIST_N; }
    __host__ __device__ int* n_cand() const { return reinterpret_cast<int*>(counters + CTR_N_CAND); }
};

// Category axis (cv_decode_cat_f32): category k's workspace is a carve of the single-category layout `ws` bytes behind
// category k - 1's, its grids `cells` cells and its predictions `n` points behind (scan points and class input shared).
// K = 1 (cv_decode_f32): k = 0, every offset is zero.
struct CatStride { int64_t ws, n, cells; };
template <class T>
__device__ __forceinline__ void cat_shift(T*& p, int64_t bytes) {
    p = (T*)((char*)p + bytes);
}
__device__ __forceinline__ Ws cat(Ws w, int64_t stride, int k) {
    const int64_t o = (int64_t)k * stride;
    cat_shift(w.L.val, o); cat_shift(w.L.xy, o); cat_shift(w.L.z, o); cat_shift(w.L.geo, o);
    cat_shift(w.counters, o); cat_shift(w.cands, o); cat_shift(w.stats, o);
    return w;
}

// workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every outstanding GLOBAL access
// (vmcnt(0)): with the candidate records stored from inside the greedy loop each barrier then cost a store round
// trip to L2 (~2 us per candidate).  Nothing the loop communicates between threads goes through global memory.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

__device__ __forceinline__ int lanes_below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// (the kernels' bodies are device functions: the category axis and the scene axis differ only in where a workgroup's
// operands come from - offsets of one set of arguments, or a row of a job table)
__device__ __forceinline__ void compact_body(const float* __restrict__ g_obj, const float* __restrict__ g_rot,
                                             const float* __restrict__ g_scale, const Geo& geo, int64_t G, float thresh,
                                             const Ws& w) {
    const List& L = w.L;
    unsigned* list_n = w.list_n();
    for (int64_t base = blockIdx.x * 256ll; base < G; base += (int64_t)gridDim.x * 256) {
        const int64_t i = base + threadIdx.x;
        float v = 0.f;
        bool hit = false;
        if (i < G) { v = g_obj[i]; hit = v >= thresh; }
        const uint64_t m = __ballot(hit);
        if (m == 0) continue;
        unsigned pos = 0;
        const int lane = threadIdx.x & 63;
        const int leader = __ffsll((unsigned long long)m) - 1;
        if (lane == leader) pos = atomicAdd(list_n, (unsigned)__popcll(m));
        pos = __shfl(pos, leader);
        if (hit) {
            const unsigned p = pos + lanes_below(m);
            const int id = (int)i;
            L.val[p] = v;
            const int z = id % geo.Z, y = (id / geo.Z) % geo.Y, x = id / (geo.Z * geo.Y);
            L.xy[p] = (unsigned)x | ((unsigned)y << 16);
            L.z[p] = z;
            const float r0 = g_rot[(int64_t)id * 2], r1 = g_rot[(int64_t)id * 2 + 1];
            const float rot = (float)atan2((double)r1, (double)r0);                            // :214
            L.geo[0 * L.cap + p] = (float)cos((double)rot);
            L.geo[1 * L.cap + p] = (float)sin((double)rot);
            for (int k = 0; k < 3; ++k) L.geo[(2 + k) * L.cap + p] = g_scale[(int64_t)id * 3 + k];   // :216
        }
    }
}

__global__ __launch_bounds__(256) void dec_compact(const float* __restrict__ g_obj,
                                                   const float* __restrict__ g_rot,
                                                   const float* __restrict__ g_scale, Geo geo,
                                                   int64_t G, float thresh, Ws w, CatStride ks) {
    const int kc = blockIdx.y;
    g_obj = g_obj + kc * ks.cells; g_rot = g_rot + kc * 2 * ks.cells; g_scale = g_scale + kc * 3 * ks.cells;
    w = cat(w, ks.ws, kc);
    compact_body(g_obj, g_rot, g_scale, geo, G, thresh, w);
}

// in-box test shared by grid suppression and back-projection:
// ((d @ R) / s) strictly inside (-1,1)^3 with R = [[c,0,-s],[0,1,0],[s,0,c]].
__device__ __forceinline__ bool inv_coords(float d0, float d1, float d2, float c, float s,
                                           const float* sc, float& w0, float& w1, float& w2) {
    w0 = fmaf(d2, s, fmaf(d1, 0.f, d0 * c)) / sc[0];
    w1 = fmaf(d2, 0.f, fmaf(d1, 1.f, d0 * 0.f)) / sc[1];
    w2 = fmaf(d2, c, fmaf(d1, 0.f, d0 * (-s))) / sc[2];
    return -1 < w0 && w0 < 1 && -1 < w1 && w1 < 1 && -1 < w2 && w2 < 1;
}

// the same test as a boolean without the three divisions (the greedy walk only needs "inside or not"): for finite
// operands -1 < RN(t / s) < 1 holds exactly when |t| < |s| - a quotient below one cannot round up to one (t <= |s| - ulp
// gives t / |s| <= 1 - 2^-24, representable), |t| >= |s| gives a quotient >= 1; s = 0, infinities and NaNs fall on the
// same side in both forms.  Bit-identical verdicts, ~30 of the ~60 vector instructions of a kill test gone.
__device__ __forceinline__ bool inside_box(float d0, float d1, float d2, float c, float s, const float* sc) {
    const float t0 = fmaf(d2, s, fmaf(d1, 0.f, d0 * c));
    const float t1 = fmaf(d2, 0.f, fmaf(d1, 1.f, d0 * 0.f));
    const float t2 = fmaf(d2, c, fmaf(d1, 0.f, d0 * (-s)));
    return fabsf(t0) < fabsf(sc[0]) && fabsf(t1) < fabsf(sc[1]) && fabsf(t2) < fabsf(sc[2]);
}

// the eight box corners relative to the centre (:217-219): bb[q][k]
__device__ __forceinline__ void box_corners(float cs, float sn, const float* sc, float* bb) {
    // raw corner signs (:217); literals so that the unrolled loop folds them (no constant-memory loads on the
    // greedy loop's critical path)
    constexpr float kRawX[8] = {1, 1, -1, -1, 1, 1, -1, -1};
    constexpr float kRawY[8] = {1, 1, 1, 1, -1, -1, -1, -1};
    constexpr float kRawZ[8] = {1, -1, -1, 1, 1, -1, -1, 1};
    const float m00 = cs * sc[0], m02 = (-sn) * sc[2], m11 = sc[1], m20 = sn * sc[0], m22 = cs * sc[2];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        bb[q * 3 + 0] = m00 * kRawX[q] + m02 * kRawZ[q];
        bb[q * 3 + 1] = m11 * kRawY[q];
        bb[q * 3 + 2] = m20 * kRawX[q] + m22 * kRawZ[q];
    }
}

struct Best {
    float v;
    int id, pos;
    int q;      // the wave that published it
};

__device__ __forceinline__ void take_better(Best& b, float v, int id, int pos, int q) {
    if (v > b.v || (v == b.v && id < b.id)) { b.v = v; b.id = id; b.pos = pos; b.q = q; }
}

constexpr int GREEDY_T = 512;        // threads of the greedy workgroup: two waves per SIMD (256: 0.180 ms, 512: 0.158 ms, 1024: 0.181 ms
                                     // decode stage at 80k points, profiles/r4/dec_small_t.txt).  One wave per SIMD runs the
                                     // per-candidate part every wave repeats - reduction, candidate set-up - once per SIMD, but
                                     // leaves the LDS round trips of a region's box tests (~1 000 per candidate at 80k points, 4 per
                                     // thread) with nothing to hide behind
constexpr int GREEDY_CAP = 4096;     // list entries held in LDS (28 bytes each)

// cross-lane moves on the DPP path (one VALU instruction, no LDS round trip): quad swaps, then row rotations leave
// every lane of a 16-lane row with the row's result; the four rows are combined through scalar registers
template <int CTRL>
__device__ __forceinline__ int dpp_mov(int x) {
    return __builtin_amdgcn_update_dpp(x, x, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ float wave_max_f32(float x) {
    x = fmaxf(x, __int_as_float(dpp_mov<0xB1>(__float_as_int(x))));     // quad_perm [1,0,3,2]
    x = fmaxf(x, __int_as_float(dpp_mov<0x4E>(__float_as_int(x))));     // quad_perm [2,3,0,1]
    x = fmaxf(x, __int_as_float(dpp_mov<0x124>(__float_as_int(x))));    // row_ror:4
    x = fmaxf(x, __int_as_float(dpp_mov<0x128>(__float_as_int(x))));    // row_ror:8
    const int xi = __float_as_int(x);
    const float a = __int_as_float(__builtin_amdgcn_readlane(xi, 0)), b = __int_as_float(__builtin_amdgcn_readlane(xi, 16)),
                c = __int_as_float(__builtin_amdgcn_readlane(xi, 32)), d = __int_as_float(__builtin_amdgcn_readlane(xi, 48));
    return fmaxf(fmaxf(a, b), fmaxf(c, d));
}
__device__ __forceinline__ int wave_min_i32(int x) {
    x = min(x, dpp_mov<0xB1>(x));
    x = min(x, dpp_mov<0x4E>(x));
    x = min(x, dpp_mov<0x124>(x));
    x = min(x, dpp_mov<0x128>(x));
    return min(min(__builtin_amdgcn_readlane(x, 0), __builtin_amdgcn_readlane(x, 16)),
               min(__builtin_amdgcn_readlane(x, 32), __builtin_amdgcn_readlane(x, 48)));
}

// The argmax of a pass over the workgroup (largest value, lowest flat index on ties: eval_joint.py:205), from every thread's
// own best: the wave's best through DPP, one LDS slot per wave, ONE barrier, then every thread reads the W slots.  The slots
// are double-buffered by the parity of `it`: the one barrier also frees the other buffer.  `also` runs in the lane that
// publishes its wave's best, before the barrier (the sorted walk sends the winner's cell along).
template <int W, class Also>
__device__ __forceinline__ Best best_of_workgroup(float (&s_val)[2][W], int (&s_idx)[2][W], int (&s_pos)[2][W], int it, float bv,
                                                  int bid, int bpos, Also&& also) {
    const int wave = threadIdx.x >> 6, par = it & 1;
    const float wv = wave_max_f32(bv);
    const int wid = wave_min_i32(bv == wv ? bid : 0x7fffffff);
    if (bv == wv && bid == wid) {
        s_val[par][wave] = bv; s_idx[par][wave] = bid; s_pos[par][wave] = bpos;
        also(par, wave);
    }
    lds_barrier();
    Best w{s_val[par][0], s_idx[par][0], s_pos[par][0], 0};
#pragma unroll
    for (int q = 1; q < W; ++q) take_better(w, s_val[par][q], s_idx[par][q], s_pos[par][q], q);
    return w;
}
template <int W>
__device__ __forceinline__ Best best_of_workgroup(float (&s_val)[2][W], int (&s_idx)[2][W], int (&s_pos)[2][W], int it, float bv,
                                                  int bid, int bpos) {
    return best_of_workgroup(s_val, s_idx, s_pos, it, bv, bid, bpos, [](int, int) {});
}

// The suppression a candidate applies to the grid - the +-elimination cube (:211) and the cells inside its oriented box
// (:225-229, :243) - as the walks test list entries against it.  Every thread holds the same values.
struct Suppress {
    int c[3] = {0, 0, 0}, clo[3] = {0, 0, 0}, chi[3] = {0, 0, 0};
    // conservative region (cube and box bounds together): one unsigned compare per axis dismisses the entries that are
    // nowhere near
    int rlo[3] = {0, 0, 0};
    unsigned rsp[3] = {0, 0, 0};
    float cs = 0.f, sn = 0.f, sc[3] = {1.f, 1.f, 1.f};
    int e, hp;
    float res;

    __device__ __forceinline__ Suppress(const Geo& geo, const cv_decode_params& prm)
        : e(prm.elimination), hp(prm.elimination + (prm.elim_hi_plus1 ? 1 : 0)), res(geo.res) {}

    __device__ __forceinline__ bool near(int x, int y, int z) const {
        // (three compares and two ANDs, no branch: a short circuit here would put a walk's load of z behind the test of x)
        return ((unsigned)(x - rlo[0]) <= rsp[0]) & ((unsigned)(y - rlo[1]) <= rsp[1]) & ((unsigned)(z - rlo[2]) <= rsp[2]);
    }
    __device__ __forceinline__ bool kills(int x, int y, int z) const {
        bool kill = x >= c[0] - e && x < c[0] + hp && y >= c[1] - e && y < c[1] + hp && z >= c[2] - e && z < c[2] + hp;
        if (!kill && x >= clo[0] && x <= chi[0] && y >= clo[1] && y <= chi[1] && z >= clo[2] && z <= chi[2]) {
            const float v0 = (float)(x - c[0]) * res, v1 = (float)(y - c[1]) * res, v2 = (float)(z - c[2]) * res;
            kill = inside_box(v0, v1, v2, cs, sn, sc);
        }
        return kill;
    }

    // Candidate `it` is the cell (xy, z) with flat index id: its box from the five geometry words g[q * gs + pos] of its
    // list position, the cells that box can reach, the candidate record (thread 0) and its zeroed statistics (the
    // workspace is not cleared by a launch).  T: threads of the workgroup, all of which call this.
    template <int T>
    __device__ __forceinline__ void take(int it, int id, unsigned xy, int z, const float* g, int64_t gs, int pos,
                                         const Geo& geo, float inv_res, Cand* __restrict__ cands, Stats* __restrict__ stats) {
        c[0] = (int)(xy & 0xffffu); c[1] = (int)(xy >> 16); c[2] = z;
        cs = g[0 * gs + pos];
        sn = g[1 * gs + pos];
        for (int k = 0; k < 3; ++k) sc[k] = g[(2 + k) * gs + pos];
        // extent of the eight corners (+-m00 +- m02, +-m11, +-m20 +- m22; :217-219): every sign combination occurs and
        // rounding is symmetric, so max = |.| + |.| and min = -max, bit for bit what the min / max over the corners give
        float hi[3];
        {
            const float m00 = cs * sc[0], m02 = (-sn) * sc[2], m11 = sc[1], m20 = sn * sc[0], m22 = cs * sc[2];
            hi[0] = fabsf(m00) + fabsf(m02);
            hi[1] = fabsf(m11);
            hi[2] = fabsf(m20) + fabsf(m22);
        }
        const int shape[3] = {geo.X, geo.Y, geo.Z};
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                             // :220-223
            const int blo = (int)((-hi[k]) * inv_res), bhi = (int)(hi[k] * inv_res);
            clo[k] = min(max(c[k] + blo, 0), shape[k] - 1);
            chi[k] = min(max(c[k] + bhi, 0), shape[k] - 1);
            rlo[k] = min(c[k] - e, clo[k]);
            rsp[k] = (unsigned)(max(c[k] + hp - 1, chi[k]) - rlo[k]);
        }
        if (threadIdx.x == 0) {
            Cand cd;
            cd.idx = id;
            for (int k = 0; k < 3; ++k) {
                cd.c[k] = c[k]; cd.clo[k] = clo[k]; cd.chi[k] = chi[k];
                cd.cw[k] = geo.corner[k] + geo.res * (float)c[k];                 // :206
                cd.sc[k] = sc[k];
            }
            cd.cs = cs; cd.sn = sn;
            cands[it] = cd;
        }
        for (int q = threadIdx.x; q < (int)(sizeof(Stats) / 4); q += T)
            reinterpret_cast<unsigned*>(&stats[it])[q] = 0u;
    }
};

// ---- The three walks.  Each runs in ONE workgroup: a pass applies the suppression of the current candidate to the live
// entries and takes the argmax of what is left; the loop ends when that drops below thresh_high (:208-209) or at max_iters.

// Lists up to GREEDY_CAP entries: the thread's entries live in registers (loaded once: a pass is VALU work only), the rare
// by-index reads go to an LDS copy.  (The first version walked the entries in LDS - two dependent LDS round trips per
// entry with one wave per SIMD and nothing to overlap them with: 10k cycles per pass for 13 entries per thread.)
__device__ __forceinline__ void walk_lds(const Geo& geo, const cv_decode_params& prm, const Ws& w, int n) {
    constexpr int T = GREEDY_T, E = GREEDY_CAP / T;      // E entries per thread
    __shared__ unsigned l_xy[GREEDY_CAP];
    __shared__ int l_z[GREEDY_CAP];
    __shared__ float l_geo[5][GREEDY_CAP];
    __shared__ float s_val[2][T / 64];
    __shared__ int s_idx[2][T / 64], s_pos[2][T / 64];
    const List& L = w.L;
    float r_val[E];
    unsigned r_xy[E], dead = 0;
    int r_z[E], r_id[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int k = (int)threadIdx.x + j * T;
        const bool ok = k < n;
        r_val[j] = ok ? L.val[k] : 0.f;
        r_xy[j] = ok ? L.xy[k] : 0u;
        r_z[j] = ok ? L.z[k] : 0;
        r_id[j] = cell_id(geo, r_xy[j], r_z[j]);
        dead |= ok ? 0u : (1u << j);
        if (ok) {
            l_xy[k] = r_xy[j];
            l_z[k] = r_z[j];
            for (int q = 0; q < 5; ++q) l_geo[q][k] = L.geo[q * L.cap + k];
        }
    }
    __syncthreads();
    const float inv_res = 1.0f / geo.res;
    Suppress s(geo, prm);
    bool have_cur = false;       // none before the first pass
    int it = 0;
    bool truncated = false;
    for (;; ++it) {
        if (have_cur) {
            unsigned near = 0;        // alive entries inside the conservative region
#pragma unroll
            for (int j = 0; j < E; ++j)
                near |= s.near((int)(r_xy[j] & 0xffffu), (int)(r_xy[j] >> 16), r_z[j]) ? (1u << j) : 0u;
            near &= ~dead;
            while (near) {            // rare: a handful of entries per candidate, taken from LDS by index
                const int j = __ffs(near) - 1;
                near &= near - 1;
                const int k = (int)threadIdx.x + j * T;
                const unsigned xy = l_xy[k];
                if (s.kills((int)(xy & 0xffffu), (int)(xy >> 16), l_z[k])) dead |= 1u << j;
            }
        }
        float bv = -1.f;
        int bpos = -1, bid = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const bool alive = !((dead >> j) & 1u);
            const float v = r_val[j];
            const int id = r_id[j];
            if (alive && (v > bv || (v == bv && id < bid))) { bv = v; bid = id; bpos = (int)threadIdx.x + j * T; }
        }
        const Best b = best_of_workgroup(s_val, s_idx, s_pos, it, bv, bid, bpos);
        if (!(b.v >= prm.thresh_high)) break;                                   // :208-209
        if (it >= prm.max_iters) { truncated = true; break; }
        s.take<T>(it, b.id, l_xy[b.pos], l_z[b.pos], &l_geo[0][0], GREEDY_CAP, b.pos, geo, inv_res, w.cands, w.stats);
        have_cur = true;
    }
    if (threadIdx.x == 0) { w.n_cand()[0] = it; w.n_cand()[1] = truncated ? 1 : 0; }
}

// Lists of any length: everything from the global arrays (L2-resident); a suppressed entry's value is zeroed in the list.
template <int T>
__device__ __forceinline__ void walk_global(const Geo& geo, const cv_decode_params& prm, const Ws& w, int n) {
    __shared__ float s_val[2][T / 64];
    __shared__ int s_idx[2][T / 64], s_pos[2][T / 64];
    const List& L = w.L;
    const float inv_res = 1.0f / geo.res;
    auto id_at = [&](int pos) { return cell_id(geo, L.xy[pos], L.z[pos]); };
    Suppress s(geo, prm);
    bool have_cur = false;
    int it = 0;
    bool truncated = false;
    for (;; ++it) {
        float bv = -1.f;
        int bpos = -1;
        for (int k = threadIdx.x; k < n; k += T) {
            const float v = L.val[k];
            if (v == 0.f) continue;
            if (have_cur) {
                const unsigned xy = L.xy[k];
                const int z = L.z[k];
                const int x = (int)(xy & 0xffffu), y = (int)(xy >> 16);
                if (s.near(x, y, z)) {
                    if (s.kills(x, y, z)) {
                        L.val[k] = 0.f;
                        continue;
                    }
                }
            }
            if (v > bv || (v == bv && id_at(k) < id_at(bpos))) { bv = v; bpos = k; }
        }
        const int bid = bpos >= 0 ? id_at(bpos) : 0x7fffffff;
        const Best b = best_of_workgroup(s_val, s_idx, s_pos, it, bv, bid, bpos);
        if (!(b.v >= prm.thresh_high)) break;                                   // :208-209
        if (it >= prm.max_iters) { truncated = true; break; }
        s.take<T>(it, b.id, L.xy[b.pos], L.z[b.pos], L.geo, L.cap, b.pos, geo, inv_res, w.cands, w.stats);
        have_cur = true;
    }
    if (threadIdx.x == 0) { w.n_cand()[0] = it; w.n_cand()[1] = truncated ? 1 : 0; }
}

// The big grids' walk (round 4).  walk_lds tests every entry of every thread against every candidate and re-scans them for
// the maximum: ~44 vector instructions per entry and pass, which is what a 300k-point scene's walk spent its 1.6 ms on
// (21 000 listed cells x 180 candidates on ONE CU).  Here
//   * a wave owns 64 * E CONSECUTIVE list entries (dec_compact appends in rounds of the grid-stride loop: a stretch of the
//     list is a window of x slabs) and every thread keeps the bounding box of its own: a candidate's suppression region is
//     tested against the box first, and a wave whose 64 boxes all miss skips its entries altogether;
//   * the entries are sorted once (value descending, flat index ascending: the order the walk takes them in), so the
//     thread's best live entry is the lowest clear bit of `dead`; value / cell / list position of that entry sit in
//     registers and are re-picked (select chains over the E slots) only when it dies;
//   * the winner's cell travels through LDS from its owner's registers - no LDS copy of the list (walk_lds's 112 KB), no
//     by-index global reads except the five geometry words.
// Same candidates in the same order as the reference loop (eval_joint.py:204-263).  A 300k-point scene's decode 1.88 ->
// 1.28 ms (LABNOTES, "Decode at 300k points", also for what is left there).  NOT used for the 80k-point lists (3 400 cells,
// 42 candidates): 0.21 ms against walk_lds's 0.18.
template <int N, class Tv>
__device__ __forceinline__ Tv pick_slot(const Tv (&r)[N], int j) {
    // slot j of a register array (a dynamic index has to become selects): a binary tree over the bits of j - N - 1 selects
    // and five bit tests, which two picks of the same j share, instead of N compares + N selects each
    static_assert(N <= 32, "five index bits");
    Tv t[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) t[i] = r[i < N ? i : N - 1];
#pragma unroll
    for (int bit = 0; bit < 5; ++bit) {
        const bool b = (j >> bit) & 1;
#pragma unroll
        for (int i = 0; i < (32 >> (bit + 1)); ++i) t[i] = b ? t[2 * i + 1] : t[2 * i];
    }
    return t[0];
}

template <int T, int E, int G>
__device__ __forceinline__ void walk_sorted(const Geo& geo, const cv_decode_params& prm, const Ws& w, int n) {
    static_assert(E >= 2 && E <= 32 && T % 64 == 0 && G % 64 == 0 && T % G == 0, "entries per thread live in one 32-bit mask");
    constexpr int W = T / 64;
    constexpr unsigned ALL = E == 32 ? 0xffffffffu : ((1u << E) - 1u);
    __shared__ float s_val[2][W];
    __shared__ int s_idx[2][W], s_pos[2][W], s_z[2][W];
    __shared__ unsigned s_xy[2][W];
    const List& L = w.L;
    // a group of G threads owns G * E consecutive list entries, dealt to its threads round-robin: the cells a candidate
    // suppresses sit next to each other in the list, and a thread that owned them all would walk them alone (E consecutive
    // entries per thread: 0.18 -> 0.30 ms at 80k points; G = 64 at 300k points: the wave that owns the ~500 suppressed cells
    // takes 9 000 cycles per candidate and the other fifteen wait)
    const int base = (int)(threadIdx.x / G) * (G * E) + (int)(threadIdx.x % G);
    float r_val[E];
    unsigned r_xy[E];
    int r_zj[E];                                   // z | j << 16: list position = base + G * j
    int bx0 = 0x7fffffff, bx1 = -1, by0 = 0x7fffffff, by1 = -1, bz0 = 0x7fffffff, bz1 = -1;
    unsigned dead;
    {
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int k = base + G * j;
            const bool ok = k < n;
            r_val[j] = ok ? L.val[k] : 0.f;
            r_xy[j] = ok ? L.xy[k] : 0u;
            const int z = ok ? L.z[k] : 0;
            r_zj[j] = z | (j << 16);
            const int x = (int)(r_xy[j] & 0xffffu), y = (int)(r_xy[j] >> 16);
            if (ok) {
                bx0 = min(bx0, x); bx1 = max(bx1, x);
                by0 = min(by0, y); by1 = max(by1, y);
                bz0 = min(bz0, z); bz1 = max(bz1, z);
                ++cnt;
            }
        }
        // odd-even transposition sort of the thread's entries (static register indices): value descending, flat index
        // ascending (computed only on a tie: no register per entry for it); the slots beyond the list (value 0) end up last
#pragma unroll
        for (int r = 0; r < E; ++r) {
#pragma unroll
            for (int j = r & 1; j + 1 < E; j += 2) {
                const float v0 = r_val[j], v1 = r_val[j + 1];
                const unsigned x0 = r_xy[j], x1 = r_xy[j + 1];
                const int z0 = r_zj[j], z1 = r_zj[j + 1];
                bool sw = v1 > v0;
                if (v1 == v0) sw = cell_id(geo, x1, z1 & 0xffff) < cell_id(geo, x0, z0 & 0xffff);
                r_val[j] = sw ? v1 : v0; r_val[j + 1] = sw ? v0 : v1;
                r_xy[j] = sw ? x1 : x0;  r_xy[j + 1] = sw ? x0 : x1;
                r_zj[j] = sw ? z1 : z0;  r_zj[j + 1] = sw ? z0 : z1;
            }
        }
        dead = ALL & ~(cnt >= 32 ? 0xffffffffu : ((1u << cnt) - 1u));
    }
    const float inv_res = 1.0f / geo.res;
    Suppress s(geo, prm);
    bool have_cur = false;
    // the thread's best live entry
    int cur_j = -1, cur_id = 0x7fffffff, cur_pos = -1, cur_z = 0;
    unsigned cur_xy = 0;
    float cur_val = -1.f;
    int it = 0;
    bool truncated = false;
    for (;; ++it) {
        // ---- suppression by the current candidate: its region against the box of the thread's entries first
        const bool hit = have_cur && dead != ALL && bx1 >= s.rlo[0] && bx0 <= s.rlo[0] + (int)s.rsp[0] && by1 >= s.rlo[1] &&
                         by0 <= s.rlo[1] + (int)s.rsp[1] && bz1 >= s.rlo[2] && bz0 <= s.rlo[2] + (int)s.rsp[2];
        if (__any(hit)) {
            if (hit) {
                unsigned near = 0;
#pragma unroll
                for (int j = 0; j < E; ++j)
                    near |= s.near((int)(r_xy[j] & 0xffffu), (int)(r_xy[j] >> 16), r_zj[j] & 0xffff) ? (1u << j) : 0u;
                near &= ~dead;
                while (near) {
                    const int j = __ffs(near) - 1;
                    near &= near - 1;
                    const unsigned xy = pick_slot<E>(r_xy, j);
                    const int z = pick_slot<E>(r_zj, j) & 0xffff;
                    if (s.kills((int)(xy & 0xffffu), (int)(xy >> 16), z)) dead |= 1u << j;
                }
            }
        }
        // ---- the thread's best live entry = the first live slot of the sorted order
        float bv = -1.f;
        int bid = 0x7fffffff, bpos = -1;
        {
            const unsigned alive = ALL & ~dead;
            if (alive != 0u) {
                if (cur_j < 0 || ((dead >> cur_j) & 1u)) {
                    cur_j = __ffs(alive) - 1;
                    cur_val = pick_slot<E>(r_val, cur_j);
                    cur_xy = pick_slot<E>(r_xy, cur_j);
                    const int zj = pick_slot<E>(r_zj, cur_j);
                    cur_z = zj & 0xffff;
                    cur_pos = base + G * (zj >> 16);
                    cur_id = cell_id(geo, cur_xy, cur_z);
                }
                bv = cur_val; bid = cur_id; bpos = cur_pos;
            }
        }
        const Best b = best_of_workgroup(s_val, s_idx, s_pos, it, bv, bid, bpos,
                                         [&](int par, int wave) { s_xy[par][wave] = cur_xy; s_z[par][wave] = cur_z; });
        if (!(b.v >= prm.thresh_high)) break;                                   // :208-209
        if (it >= prm.max_iters) { truncated = true; break; }
        s.take<T>(it, b.id, s_xy[it & 1][b.q], s_z[it & 1][b.q], L.geo, L.cap, b.pos, geo, inv_res, w.cands, w.stats);
        have_cur = true;
    }
    if (threadIdx.x == 0) { w.n_cand()[0] = it; w.n_cand()[1] = truncated ? 1 : 0; }
}

// One walker workgroup per category (blockIdx.y): the K walks run side by side.  The list length is only known on the
// device, so the kernel picks the walk: lists up to GREEDY_CAP entries in registers + LDS, longer ones over the global arrays
__device__ __forceinline__ void greedy_body(const Geo& geo, const cv_decode_params& prm, const Ws& w) {
    const unsigned n = *w.list_n();
    if (n <= (unsigned)GREEDY_CAP) walk_lds(geo, prm, w, (int)n);
    else walk_global<GREEDY_T>(geo, prm, w, (int)n);
}
__global__ __launch_bounds__(GREEDY_T) void dec_greedy_dispatch(Geo geo, cv_decode_params prm, Ws w, int64_t ks_ws) {
    w = cat(w, ks_ws, blockIdx.y);
    greedy_body(geo, prm, w);
}
// big grids (the host picks this launch from the cell count): 1024 threads, lists up to 24576 cells in registers (a
// 300k-point scene lists ~21 000 cells) on the sorted walk
constexpr int GREEDY_T_BIG = 1024;
constexpr int GREEDY_E_BIG = 24;
constexpr int GREEDY_G_BIG = 64;
__device__ __forceinline__ void greedy_big_body(const Geo& geo, const cv_decode_params& prm, const Ws& w) {
    const unsigned n = *w.list_n();
    if (n <= (unsigned)(GREEDY_E_BIG * GREEDY_T_BIG)) walk_sorted<GREEDY_T_BIG, GREEDY_E_BIG, GREEDY_G_BIG>(geo, prm, w, (int)n);
    else walk_global<GREEDY_T_BIG>(geo, prm, w, (int)n);
}
__global__ __launch_bounds__(GREEDY_T_BIG) void dec_greedy_dispatch_big(Geo geo, cv_decode_params prm, Ws w, int64_t ks_ws) {
    w = cat(w, ks_ws, blockIdx.y);
    greedy_big_body(geo, prm, w);
}

// packed host result: [0]=n_cand [1]=n_boxes [2]=truncated, then arrays sized by max_iters
struct ResultLayout {
    size_t off_cand, off_verdict, off_boxes, off_scores, off_classes, total;
    __host__ __device__ explicit ResultLayout(int M) {
        size_t o = 16;
        off_cand = o; o += sizeof(long long) * M;
        off_verdict = o; o += sizeof(int) * M;
        off_boxes = o; o += sizeof(float) * 24 * M;
        off_scores = o; o += sizeof(float) * M;
        off_classes = o; o += sizeof(int) * M;
        total = cv_align_up(o, 16);
    }
};

// verdicts (:246-253), class mode (:255-256) and box corners (:258): one thread per candidate, accepted boxes
// written in candidate order (acceptance order of the sequential loop)
__device__ void finalize_block(const Cand* __restrict__ cands, const Stats* __restrict__ stats, int nc,
                               int truncated, cv_decode_params prm, char* result, int M, int* s_scan /*[256]*/) {
    const ResultLayout L(M);
    int* hdr = reinterpret_cast<int*>(result);
    long long* o_cand = reinterpret_cast<long long*>(result + L.off_cand);
    int* o_verdict = reinterpret_cast<int*>(result + L.off_verdict);
    float* o_boxes = reinterpret_cast<float*>(result + L.off_boxes);
    float* o_scores = reinterpret_cast<float*>(result + L.off_scores);
    int* o_classes = reinterpret_cast<int*>(result + L.off_classes);
    int base = 0;
    for (int k0 = 0; k0 < nc; k0 += 256) {
        const int k = k0 + (int)threadIdx.x;
        int verdict = -1, best = 0;
        if (k < nc) {
            const Stats& s = stats[k];
            const float lhs = (float)s.n_mask, rhs = prm.valid_ratio * (float)s.n_in;
            if (lhs < rhs || (float)s.n_in < prm.thresh_low) verdict = 1;               // :246-247
            else {
                const float error = (float)(s.err / (double)s.n_mask);
                if ((double)error > prm.err_thresh) verdict = 2;                         // :252-253
                else {
                    verdict = 0;
                    unsigned best_cnt = s.hist[0];
                    for (int c = 1; c < NCLS; ++c)
                        if (s.hist[c] > best_cnt) { best_cnt = s.hist[c]; best = c; }
                }
            }
            o_cand[k] = cands[k].idx;
            o_verdict[k] = verdict;
        }
        // exclusive scan of the accepted flags over the 256 threads
        s_scan[threadIdx.x] = verdict == 0 ? 1 : 0;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int add = (int)threadIdx.x >= off ? s_scan[threadIdx.x - off] : 0;
            __syncthreads();
            s_scan[threadIdx.x] += add;
            __syncthreads();
        }
        const int incl = s_scan[threadIdx.x], total = s_scan[255];
        if (verdict == 0) {
            const int nb = base + incl - 1;
            const Cand& cd = cands[k];
            float bb[24];
            box_corners(cd.cs, cd.sn, cd.sc, bb);
            for (int q = 0; q < 8; ++q)
                for (int d = 0; d < 3; ++d) o_boxes[(size_t)nb * 24 + q * 3 + d] = bb[q * 3 + d] + cd.cw[d];  // :258
            o_scores[nb] = __uint_as_float(stats[k].pmax_bits);
            o_classes[nb] = best;
        }
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) { hdr[0] = nc; hdr[1] = base; hdr[2] = truncated; hdr[3] = 0; }
}

// (blockIdx.x: 256 points; blockIdx.y strides over the candidate groups)
__device__ __forceinline__ void backproject_body(const float* __restrict__ pts, const float* __restrict__ xyz,
                                                 const float* __restrict__ prob, const int* __restrict__ cls, int64_t n,
                                                 float prob_thresh, const Ws& w) {
    const Cand* cands = w.cands;
    Stats* stats = w.stats;
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    const bool have = i < n;
    float p0 = 0, p1 = 0, p2 = 0, x0 = 0, x1 = 0, x2 = 0, pr = 0;
    int cl = 0;
    if (have) {
        p0 = pts[i * 3]; p1 = pts[i * 3 + 1]; p2 = pts[i * 3 + 2];
        x0 = xyz[i * 3]; x1 = xyz[i * 3 + 1]; x2 = xyz[i * 3 + 2];
        pr = prob[i];
        cl = cls ? cls[i] : 0;          // (no class input: class 0, separate mode)
    }
    const int nc = w.n_cand()[0];
    // A workgroup takes its 256 points through GROUPS of CB candidates (blockIdx.y, strided): with all candidates
    // in one workgroup the launch had 1.2 waves per SIMD, each walking 42 dependent (LDS read -> three IEEE
    // divisions -> LDS atomics) rounds on its own - 46 us for 3.4 M in-box tests.  Candidates are staged through
    // LDS (a dependent L2 load per candidate per wave dominated the first version).
    constexpr int CB = 8;
    __shared__ float c_cw[CB][3], c_sc[CB][3], c_cs[CB], c_sn[CB];
    // per-workgroup statistics in LDS, flushed once per candidate group: thousands of waves adding to
    // the same five global words per candidate serialise at ~11 ns per atomic (93 us for 42 candidates).
    // The lanes inside a box add to them directly: scan order is not spatial, so most waves hold one or two points
    // of most boxes, and a wave-level reduction (18 cross-lane moves per candidate for those one or two lanes) cost
    // several times the handful of LDS atomics it saved
    __shared__ unsigned l_in[CB], l_mask[CB], l_pmax[CB], l_hist[CB][NCLS];
    __shared__ double l_err[CB];
    for (int k0 = blockIdx.y * CB; k0 < nc; k0 += gridDim.y * CB) {
        const int nb = min(CB, nc - k0);
        __syncthreads();
        if (threadIdx.x < nb) {
            const Cand& cd = cands[k0 + threadIdx.x];
            for (int d = 0; d < 3; ++d) { c_cw[threadIdx.x][d] = cd.cw[d]; c_sc[threadIdx.x][d] = cd.sc[d]; }
            c_cs[threadIdx.x] = cd.cs;
            c_sn[threadIdx.x] = cd.sn;
        }
        if (threadIdx.x < CB) { l_in[threadIdx.x] = 0; l_mask[threadIdx.x] = 0; l_pmax[threadIdx.x] = 0; l_err[threadIdx.x] = 0.0; }
        for (int e = threadIdx.x; e < nb * NCLS; e += 256) (&l_hist[0][0])[e] = 0;
        __syncthreads();
        if (have)
            for (int kk = 0; kk < nb; ++kk) {
                float w0, w1, w2;
                if (!inv_coords(p0 - c_cw[kk][0], p1 - c_cw[kk][1], p2 - c_cw[kk][2], c_cs[kk], c_sn[kk], c_sc[kk],
                                w0, w1, w2))                                                 // :231-234
                    continue;
                atomicAdd(&l_in[kk], 1u);
                atomicMax(&l_pmax[kk], __float_as_uint(pr));       // prob >= 0: bit order == value order
                if (pr > prob_thresh) {                                                       // :245
                    const float e0 = x0 - w0, e1 = x1 - w1, e2 = x2 - w2;
                    const float ss = (e0 * e0 + e1 * e1) + e2 * e2;
                    atomicAdd(&l_mask[kk], 1u);
                    __hip_atomic_fetch_add(&l_err[kk], (double)(sqrtf(ss) * pr), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);                     // :250
                    if ((unsigned)cl < (unsigned)NCLS) atomicAdd(&l_hist[kk][cl], 1u);
                }
            }
        __syncthreads();
        if (threadIdx.x < nb && l_in[threadIdx.x]) {
            const int k = k0 + threadIdx.x;
            atomicAdd(&stats[k].n_in, l_in[threadIdx.x]);
            if (l_mask[threadIdx.x]) {
                atomicAdd(&stats[k].n_mask, l_mask[threadIdx.x]);
                atomicAdd(&stats[k].err, l_err[threadIdx.x]);
            }
            atomicMax(&stats[k].pmax_bits, l_pmax[threadIdx.x]);
        }
        for (int e = threadIdx.x; e < nb * NCLS; e += 256) {
            const unsigned v = l_hist[e / NCLS][e % NCLS];
            if (v) atomicAdd(&stats[k0 + e / NCLS].hist[e % NCLS], v);
        }
    }
}

__global__ __launch_bounds__(256) void dec_backproject(
    const float* __restrict__ pts, const float* __restrict__ xyz, const float* __restrict__ prob,
    const int* __restrict__ cls, int64_t n, float prob_thresh, Ws w, CatStride ks) {
    // category: blockIdx.z
    const int kc = blockIdx.z;
    xyz = xyz + kc * 3 * ks.n; prob = prob + kc * ks.n;
    w = cat(w, ks.ws, kc);
    backproject_body(pts, xyz, prob, cls, n, prob_thresh, w);
}

// one launch boundary (~2 us) instead of a release fence in each of the thousands of back-projection workgroups (an
// agent-scope release writes the XCD's L2 back: the fused version ran 4x slower)
__global__ __launch_bounds__(256) void dec_finalize(Ws w, cv_decode_params prm, char* result, int M, int64_t ks_ws,
                                                    int64_t result_stride) {
    w = cat(w, ks_ws, blockIdx.y);
    result += (int64_t)blockIdx.y * result_stride;
    __shared__ int s_scan[256];
    finalize_block(w.cands, w.stats, w.n_cand()[0], w.n_cand()[1], prm, result, M, s_scan);
}

// optional: replay the zeroing on the real grid (the reference mutates grid_obj in place)
__device__ __forceinline__ void apply_body(float* __restrict__ g_obj, const Geo& geo, const cv_decode_params& prm,
                                           const Ws& w) {
    const int k = blockIdx.x;
    if (k >= w.n_cand()[0]) return;
    const Cand& cd = w.cands[k];
    const int e = prm.elimination, hp = e + (prm.elim_hi_plus1 ? 1 : 0);
    {
        const int x0 = max(cd.c[0] - e, 0), y0 = max(cd.c[1] - e, 0), z0 = max(cd.c[2] - e, 0);
        const int x1 = min(cd.c[0] + hp, geo.X), y1 = min(cd.c[1] + hp, geo.Y),
                  z1 = min(cd.c[2] + hp, geo.Z);
        const int nx = max(x1 - x0, 0), ny = max(y1 - y0, 0), nz = max(z1 - z0, 0);
        for (int t = threadIdx.x; t < nx * ny * nz; t += 256) {
            const int z = z0 + t % nz, y = y0 + (t / nz) % ny, x = x0 + t / (nz * ny);
            g_obj[((int64_t)x * geo.Y + y) * geo.Z + z] = 0.f;
        }
    }
    const int nx = cd.chi[0] - cd.clo[0] + 1, ny = cd.chi[1] - cd.clo[1] + 1,
              nz = cd.chi[2] - cd.clo[2] + 1;
    for (int64_t t = threadIdx.x; t < (int64_t)nx * ny * nz; t += 256) {
        const int z = cd.clo[2] + (int)(t % nz), y = cd.clo[1] + (int)((t / nz) % ny),
                  x = cd.clo[0] + (int)(t / ((int64_t)nz * ny));
        float w0, w1, w2;
        if (inv_coords((float)(x - cd.c[0]) * geo.res, (float)(y - cd.c[1]) * geo.res,
                       (float)(z - cd.c[2]) * geo.res, cd.cs, cd.sn, cd.sc, w0, w1, w2))
            g_obj[((int64_t)x * geo.Y + y) * geo.Z + z] = 0.f;
    }
}

__global__ __launch_bounds__(256) void dec_apply(float* __restrict__ g_obj, Geo geo,
                                                 cv_decode_params prm, Ws w, CatStride ks) {
    g_obj = g_obj + (int64_t)blockIdx.y * ks.cells;
    w = cat(w, ks.ws, blockIdx.y);
    apply_body(g_obj, geo, prm, w);
}

// the counters of K workspace carves zeroed in one launch
__global__ __launch_bounds__(64) void dec_zero_counters(Ws w, int64_t ks_ws) {
    w = cat(w, ks_ws, blockIdx.y);
    if (threadIdx.x < CTR_WORDS) w.counters[threadIdx.x] = 0u;
}

// ---- Scene axis (cv_decode_scenes_f32): B jobs that share NOTHING but the parameters - every job has its own grid shape,
// corner, grid triple, workspace carve and row range [row0, row0 + n) of the shared point / prediction arrays.  The job
// table travels by value in the kernel arguments (16 x 144 bytes of the 4 KB) and the job index sits where the category index
// sits above.  Launch extents are the maximum over the jobs: a workgroup beyond its own job's extent returns at once.
struct SceneJob {
    Geo geo;
    int big;                 // the walker workgroup the single call would choose for this grid (CV_DEC_BIG_CELLS)
    Ws w;
    float* g_obj; const float* g_rot; const float* g_scale;
    int64_t row0, n, G;
};
struct SceneJobs { SceneJob j[CV_MAX_SCENES]; };
static_assert(sizeof(SceneJobs) + 64 <= 4096, "the job table is a kernel argument");

__global__ __launch_bounds__(64) void dec_zero_counters_scenes(SceneJobs js) {
    const SceneJob& j = js.j[blockIdx.y];
    if (threadIdx.x < CTR_WORDS) j.w.counters[threadIdx.x] = 0u;
}
__global__ __launch_bounds__(256) void dec_compact_scenes(SceneJobs js, float thresh) {
    const SceneJob& j = js.j[blockIdx.y];
    if (blockIdx.x * 256ll >= j.G) return;
    compact_body(j.g_obj, j.g_rot, j.g_scale, j.geo, j.G, thresh, j.w);
}
__global__ __launch_bounds__(GREEDY_T) void dec_greedy_dispatch_scenes(SceneJobs js, cv_decode_params prm) {
    const SceneJob& j = js.j[blockIdx.y];
    if (j.big) return;       // (the other walker's job)
    greedy_body(j.geo, prm, j.w);
}
__global__ __launch_bounds__(GREEDY_T_BIG) void dec_greedy_dispatch_big_scenes(SceneJobs js, cv_decode_params prm) {
    const SceneJob& j = js.j[blockIdx.y];
    if (!j.big) return;
    greedy_big_body(j.geo, prm, j.w);
}
__global__ __launch_bounds__(256) void dec_backproject_scenes(const float* __restrict__ pts, const float* __restrict__ xyz,
                                                              const float* __restrict__ prob, const int* __restrict__ cls,
                                                              float prob_thresh, SceneJobs js) {
    const SceneJob& j = js.j[blockIdx.z];
    if (blockIdx.x * 256ll >= j.n) return;       // (every workgroup of a job adds into that job's own statistics)
    backproject_body(pts + j.row0 * 3, xyz + j.row0 * 3, prob + j.row0, cls + j.row0, j.n, prob_thresh, j.w);
}
__global__ __launch_bounds__(256) void dec_finalize_scenes(SceneJobs js, cv_decode_params prm, char* result, int M,
                                                           int64_t result_stride) {
    const SceneJob& j = js.j[blockIdx.y];
    result += (int64_t)blockIdx.y * result_stride;
    __shared__ int s_scan[256];
    finalize_block(j.w.cands, j.w.stats, j.w.n_cand()[0], j.w.n_cand()[1], prm, result, M, s_scan);
}
__global__ __launch_bounds__(256) void dec_apply_scenes(SceneJobs js, cv_decode_params prm) {
    const SceneJob& j = js.j[blockIdx.y];
    apply_body(j.g_obj, j.geo, prm, j.w);
}

// the single-category workspace: the list arrays (one slot per grid cell), the counters block, candidates, statistics
struct WsLayout {
    size_t off_val, off_xy, off_z, off_geo, off_counters, off_cands, off_stats, total;
    int64_t cells;
    WsLayout(int64_t G, int M) : cells(G) {
        size_t o = 0;
        off_val = o; o = cv_align_up(o + sizeof(float) * G, 256);
        off_xy = o; o = cv_align_up(o + sizeof(unsigned) * G, 256);
        off_z = o; o = cv_align_up(o + sizeof(int) * G, 256);
        off_geo = o; o = cv_align_up(o + sizeof(float) * 5 * G, 256);
        off_counters = o; o = cv_align_up(o + sizeof(unsigned) * CTR_WORDS, 256);
        off_cands = o; o = cv_align_up(o + sizeof(Cand) * M, 256);
        off_stats = o; o = cv_align_up(o + sizeof(Stats) * M, 256);
        // (a result block's worth of bytes that no kernel uses since the results go to pinned host memory: still reported)
        o = cv_align_up(o + ResultLayout(M).total, 256);
        total = o;
    }
    Ws at(char* ws) const {
        Ws w;
        w.L.val = reinterpret_cast<float*>(ws + off_val);
        w.L.xy = reinterpret_cast<unsigned*>(ws + off_xy);
        w.L.z = reinterpret_cast<int*>(ws + off_z);
        w.L.geo = reinterpret_cast<float*>(ws + off_geo);
        w.L.cap = cells;
        w.counters = reinterpret_cast<unsigned*>(ws + off_counters);
        w.cands = reinterpret_cast<Cand*>(ws + off_cands);
        w.stats = reinterpret_cast<Stats*>(ws + off_stats);
        return w;
    }
};

// Pinned, device-visible host buffers the last workgroup writes the results into (no copy launch, no pageable
// staging).  A buffer is owned by one call at a time; concurrent scenes (one host thread + stream each) get their own.
struct PinnedPool {
    std::mutex mu;
    std::vector<std::pair<char*, size_t>> free_list;
    // a buffer of at least `bytes` with its capacity; {nullptr, 0} when the allocation fails
    std::pair<char*, size_t> take(size_t bytes) {
        {
            std::lock_guard<std::mutex> g(mu);
            for (size_t i = 0; i < free_list.size(); ++i)
                if (free_list[i].second >= bytes) {
                    const std::pair<char*, size_t> b = free_list[i];
                    free_list.erase(free_list.begin() + i);
                    return b;
                }
        }
        void* p = nullptr;
        if (hipHostMalloc(&p, bytes, hipHostMallocMapped) != hipSuccess) return {nullptr, 0};
        return {static_cast<char*>(p), bytes};
    }
    void give(std::pair<char*, size_t> b) {
        std::lock_guard<std::mutex> g(mu);
        if (free_list.size() < 64) free_list.push_back(b);
        else (void)hipHostFree(b.first);
    }
};
PinnedPool g_pinned;

// a pool buffer for the length of a call
struct PinnedLease {
    const std::pair<char*, size_t> buf;
    explicit PinnedLease(size_t bytes) : buf(g_pinned.take(bytes)) {}
    ~PinnedLease() { if (buf.first) g_pinned.give(buf); }
    PinnedLease(const PinnedLease&) = delete;
    PinnedLease& operator=(const PinnedLease&) = delete;
};

// block k of the pinned results into the caller's arrays at k, k * M, k * M * 24
int land_result(const DecodeCall& c, const char* hk, const ResultLayout& RL, int k, int M) {
    const int* hdr = reinterpret_cast<const int*>(hk);
    const int nc = hdr[0], nb = hdr[1];
    CV_REQUIRE(nc >= 0 && nc <= M && nb >= 0 && nb <= nc, CV_ERANGE, "corrupt decode result");
    c.h_n_cand[k] = nc;
    c.h_n_boxes[k] = nb;
    if (c.h_truncated) c.h_truncated[k] = hdr[2];
    std::memcpy(c.h_cand_idx + (size_t)k * M, hk + RL.off_cand, sizeof(int64_t) * nc);
    std::memcpy(c.h_verdict + (size_t)k * M, hk + RL.off_verdict, sizeof(int32_t) * nc);
    std::memcpy(c.h_boxes + (size_t)k * M * 24, hk + RL.off_boxes, sizeof(float) * 24 * nb);
    std::memcpy(c.h_scores + (size_t)k * M, hk + RL.off_scores, sizeof(float) * nb);
    std::memcpy(c.h_classes + (size_t)k * M, hk + RL.off_classes, sizeof(int32_t) * nb);
    return CV_OK;
}

// grids beyond this many cells take the 1024-thread walker (read once per process)
long long dec_big_cells() {
    static const long long big_cells = getenv("CV_DEC_BIG_CELLS") ? atoll(getenv("CV_DEC_BIG_CELLS")) : (4ll << 20);
    return big_cells;
}

}  // namespace

// (C++ linkage, cv_common.h) K categories; category k's host outputs at k, k * M, k * M * 24
int cv_decode_run(const DecodeCall& c, int K, bool need_class) {
    CV_REQUIRE(K >= 1 && K <= CV_MAX_CATEGORIES, CV_EINVAL, "num_cats out of range (%d, 1..%d)", K, CV_MAX_CATEGORIES);
    CV_REQUIRE(c.d_grid_obj && c.d_grid_rot && c.d_grid_scale && c.dims && c.h_corner3 && c.d_points && c.d_xyz && c.d_prob &&
                   (c.d_class || !need_class) && c.params && c.d_ws && c.h_n_cand && c.h_cand_idx && c.h_verdict && c.h_n_boxes &&
                   c.h_boxes && c.h_scores && c.h_classes,
               CV_EINVAL, "null pointer argument");
    const int* dims = c.dims;
    const cv_decode_params* params = c.params;
    const int64_t n = c.n;
    hipStream_t st = static_cast<hipStream_t>(c.stream);
    CV_REQUIRE(n > 0, CV_EINVAL, "n must be positive");
    CV_REQUIRE(c.res > 0.f, CV_EINVAL, "res must be positive");
    CV_REQUIRE(dims[0] > 0 && dims[1] > 0 && dims[2] > 0, CV_EINVAL, "bad grid dims");
    CV_REQUIRE(dims[0] < 65536 && dims[1] < 65536 && dims[2] < 65536, CV_EINVAL, "grid dims must be below 65536");
    const int64_t G = (int64_t)dims[0] * dims[1] * dims[2];
    CV_REQUIRE(G < (1ll << 31), CV_EINVAL, "grid too large");
    const int M = params->max_iters;
    CV_REQUIRE(M > 0 && M <= 65536, CV_EINVAL, "max_iters out of range");
    CV_REQUIRE(params->elimination >= 0, CV_EINVAL, "elimination must be >= 0");
    // the reference loop ends when the grid maximum drops below thresh_high (eval_joint.py:208-209); with a
    // threshold <= 0 it never ends
    CV_REQUIRE(params->thresh_high > 0.f, CV_EINVAL, "thresh_high must be positive");
    const WsLayout W(G, M);
    const size_t need = (size_t)K * W.total;
    CV_REQUIRE(c.ws_bytes >= need, CV_ENOMEM, "workspace too small (%zu < %zu)", c.ws_bytes, need);
    const Ws w = W.at(static_cast<char*>(c.d_ws));
    const ResultLayout RL(M);
    const PinnedLease lease((size_t)K * RL.total);
    char* host = lease.buf.first;
    CV_REQUIRE(host != nullptr, CV_ENOMEM, "pinned host buffer of %zu bytes", (size_t)K * RL.total);
    const CatStride ks{K > 1 ? (int64_t)W.total : 0, n, G};

    if (K == 1) CV_HIP_CHECK(hipMemsetAsync(w.counters, 0, sizeof(unsigned) * CTR_WORDS, st));
    else {
        dec_zero_counters<<<dim3(1, K), 64, 0, st>>>(w, ks.ws);
        CV_LAUNCH_CHECK();
    }
    Geo geo{dims[0], dims[1], dims[2], {c.h_corner3[0], c.h_corner3[1], c.h_corner3[2]}, c.res};
    const int cblocks = (int)std::min<int64_t>((G + 255) / 256, 2048);
    dec_compact<<<dim3(cblocks, K), 256, 0, st>>>(c.d_grid_obj, c.d_grid_rot, c.d_grid_scale, geo, G, params->thresh_high, w, ks);
    CV_LAUNCH_CHECK();
    // the walk is chosen by the kernel from the list length; the host only chooses the workgroup: grids beyond 4 M cells
    // (300k-point scenes) list more cells than the 512-thread walker keeps in registers
    if (G > dec_big_cells()) dec_greedy_dispatch_big<<<dim3(1, K), GREEDY_T_BIG, 0, st>>>(geo, *params, w, ks.ws);
    else dec_greedy_dispatch<<<dim3(1, K), GREEDY_T, 0, st>>>(geo, *params, w, ks.ws);
    CV_LAUNCH_CHECK();
    // candidate groups of 8 over blockIdx.y (the count is only known on the device: groups beyond it return at once)
    const dim3 bgrid((unsigned)((n + 255) / 256), (unsigned)std::min((M + 7) / 8, 8), (unsigned)K);
    dec_backproject<<<bgrid, 256, 0, st>>>(c.d_points, c.d_xyz, c.d_prob, c.d_class, n, params->prob_thresh, w, ks);
    CV_LAUNCH_CHECK();
    dec_finalize<<<dim3(1, K), 256, 0, st>>>(w, *params, host, M, ks.ws, (int64_t)RL.total);
    CV_LAUNCH_CHECK();
    if (c.mutate_grid) {
        dec_apply<<<dim3(M, K), 256, 0, st>>>(c.d_grid_obj, geo, *params, w, ks);
        CV_LAUNCH_CHECK();
    }
    // (the event sits in front of the host's wait, so that the stage time it closes is a device time)
    if (c.ev_done) CV_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(c.ev_done), st));
    CV_HIP_CHECK(hipStreamSynchronize(st));
    for (int k = 0; k < K; ++k) {
        const int rc = land_result(c, host + (size_t)k * RL.total, RL, k, M);
        if (rc != CV_OK) return rc;
    }
    return CV_OK;
}

// (C++ linkage, cv_common.h) B scenes; scene b's host outputs at b, b * M, b * M * 24.  c: the shared arrays, the parameters,
// the workspace (carved in job order, each job its single-call size) and the host outputs; its grid / dims / corner / n fields
// are not read (the jobs carry them).
int cv_decode_scenes_run(const DecodeCall& c, const cv_decode_scene_job* jobs, int B) {
    CV_REQUIRE(B >= 1 && B <= CV_MAX_SCENES, CV_EINVAL, "num_scenes out of range (%d, 1..%d)", B, CV_MAX_SCENES);
    CV_REQUIRE(jobs && c.d_points && c.d_xyz && c.d_prob && c.d_class && c.params && c.d_ws && c.h_n_cand && c.h_cand_idx &&
                   c.h_verdict && c.h_n_boxes && c.h_boxes && c.h_scores && c.h_classes,
               CV_EINVAL, "null pointer argument");
    const cv_decode_params* params = c.params;
    hipStream_t st = static_cast<hipStream_t>(c.stream);
    CV_REQUIRE(c.res > 0.f, CV_EINVAL, "res must be positive");
    const int M = params->max_iters;
    CV_REQUIRE(M > 0 && M <= 65536, CV_EINVAL, "max_iters out of range");
    CV_REQUIRE(params->elimination >= 0, CV_EINVAL, "elimination must be >= 0");
    CV_REQUIRE(params->thresh_high > 0.f, CV_EINVAL, "thresh_high must be positive");
    size_t need = 0;
    for (int b = 0; b < B; ++b) {
        const cv_decode_scene_job& j = jobs[b];
        CV_REQUIRE(j.d_grid_obj && j.d_grid_rot && j.d_grid_scale, CV_EINVAL, "scene %d: null grid pointer", b);
        CV_REQUIRE(j.n > 0 && j.row0 >= 0, CV_EINVAL, "scene %d: bad row range (first row %lld, %lld rows)", b, (long long)j.row0,
                   (long long)j.n);
        CV_REQUIRE(j.dims[0] > 0 && j.dims[1] > 0 && j.dims[2] > 0, CV_EINVAL, "scene %d: bad grid dims", b);
        CV_REQUIRE(j.dims[0] < 65536 && j.dims[1] < 65536 && j.dims[2] < 65536, CV_EINVAL, "scene %d: grid dims must be below 65536", b);
        CV_REQUIRE((int64_t)j.dims[0] * j.dims[1] * j.dims[2] < (1ll << 31), CV_EINVAL, "scene %d: grid too large", b);
        need += WsLayout((int64_t)j.dims[0] * j.dims[1] * j.dims[2], M).total;
    }
    CV_REQUIRE(c.ws_bytes >= need, CV_ENOMEM, "workspace too small (%zu < %zu)", c.ws_bytes, need);
    if (B == 1) {       // one scene: the single call's launches, on its row range
        const cv_decode_scene_job& j = jobs[0];
        DecodeCall one = c;
        one.d_grid_obj = j.d_grid_obj; one.d_grid_rot = j.d_grid_rot; one.d_grid_scale = j.d_grid_scale;
        one.dims = j.dims; one.h_corner3 = j.corner;
        one.d_points = c.d_points + j.row0 * 3; one.d_xyz = c.d_xyz + j.row0 * 3; one.d_prob = c.d_prob + j.row0;
        one.d_class = c.d_class + j.row0; one.n = j.n;
        return cv_decode_run(one, 1, true);
    }
    const ResultLayout RL(M);
    const PinnedLease lease((size_t)B * RL.total);
    char* host = lease.buf.first;
    CV_REQUIRE(host != nullptr, CV_ENOMEM, "pinned host buffer of %zu bytes", (size_t)B * RL.total);

    SceneJobs js;
    std::memset(&js, 0, sizeof(js));
    int64_t max_G = 0, max_n = 0;
    bool any_small = false, any_big = false;
    char* ws = static_cast<char*>(c.d_ws);
    for (int b = 0; b < B; ++b) {
        const cv_decode_scene_job& j = jobs[b];
        SceneJob& o = js.j[b];
        o.G = (int64_t)j.dims[0] * j.dims[1] * j.dims[2];
        o.geo = Geo{j.dims[0], j.dims[1], j.dims[2], {j.corner[0], j.corner[1], j.corner[2]}, c.res};
        o.big = o.G > dec_big_cells() ? 1 : 0;
        const WsLayout W(o.G, M);
        o.w = W.at(ws);
        ws += W.total;
        o.g_obj = j.d_grid_obj; o.g_rot = j.d_grid_rot; o.g_scale = j.d_grid_scale;
        o.row0 = j.row0; o.n = j.n;
        max_G = std::max(max_G, o.G);
        max_n = std::max(max_n, o.n);
        (o.big ? any_big : any_small) = true;
    }
    dec_zero_counters_scenes<<<dim3(1, B), 64, 0, st>>>(js);
    CV_LAUNCH_CHECK();
    const int cblocks = (int)std::min<int64_t>((max_G + 255) / 256, 2048);
    dec_compact_scenes<<<dim3(cblocks, B), 256, 0, st>>>(js, params->thresh_high);
    CV_LAUNCH_CHECK();
    // each scene on the walker the single call would choose for its grid: a batch on both sides of the switch is two launches
    if (any_small) {
        dec_greedy_dispatch_scenes<<<dim3(1, B), GREEDY_T, 0, st>>>(js, *params);
        CV_LAUNCH_CHECK();
    }
    if (any_big) {
        dec_greedy_dispatch_big_scenes<<<dim3(1, B), GREEDY_T_BIG, 0, st>>>(js, *params);
        CV_LAUNCH_CHECK();
    }
    const dim3 bgrid((unsigned)((max_n + 255) / 256), (unsigned)std::min((M + 7) / 8, 8), (unsigned)B);
    dec_backproject_scenes<<<bgrid, 256, 0, st>>>(c.d_points, c.d_xyz, c.d_prob, c.d_class, params->prob_thresh, js);
    CV_LAUNCH_CHECK();
    dec_finalize_scenes<<<dim3(1, B), 256, 0, st>>>(js, *params, host, M, (int64_t)RL.total);
    CV_LAUNCH_CHECK();
    if (c.mutate_grid) {
        dec_apply_scenes<<<dim3(M, B), 256, 0, st>>>(js, *params);
        CV_LAUNCH_CHECK();
    }
    if (c.ev_done) CV_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(c.ev_done), st));
    CV_HIP_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b) {
        const int rc = land_result(c, host + (size_t)b * RL.total, RL, b, M);
        if (rc != CV_OK) return rc;
    }
    return CV_OK;
}

// ---- dec_instances: which scan points each final detection owns (cv_decode_instances_f32).  The decode's dec_backproject
// forms the same membership (eval_joint.py:231-245: bbox_mask_world and mask) for every candidate before NMS and reduces it
// to five statistics; here the caller names the boxes it wants - grid cells the decode examined, in priority order - and gets
// the per-point answer.  Two launches, no host wait:
//
//   inst_boxes    one thread per (category, box): the geometry the decode gave the box's cell as a candidate (rotation and
//                 scale as dec_compact, centre as the walk's candidate step), as a 12-word record in the workspace; the box's
//                 two count words are zeroed.  The host lists travel as kernel arguments (INST_CHUNK entries per launch): they
//                 are consumed when the launch is enqueued, so the caller may reuse them at once and nothing is pinned.
//   inst_assign   one thread per scan point, category on blockIdx.y: the records of INST_GROUP boxes at a time through LDS,
//                 walked in list order; the first box that has the point as a member owns it.
namespace {

constexpr int INST_GROUP = 64;      // boxes staged in LDS at a time (3 KB of records)
constexpr int INST_REC = 12;        // words of a box record: centre xyz, cos | sin, scale xyz | label, three unused
constexpr int INST_CHUNK = 256;     // (category, box) entries of one inst_boxes launch: 3 KB of the 4 KB kernel arguments

struct InstChunk {
    int cell[INST_CHUNK];           // flat grid cell
    int label[INST_CHUNK];
    int slot[INST_CHUNK];           // k * max_boxes + j: record and count position
};
struct InstCats {
    int n_boxes[CV_MAX_CATEGORIES];
};

__global__ __launch_bounds__(INST_CHUNK) void inst_boxes(const float* __restrict__ g_rot, const float* __restrict__ g_scale,
                                                         Geo geo, int64_t cells, int max_boxes, InstChunk ch, int count,
                                                         unsigned* __restrict__ recs, int32_t* __restrict__ count_in,
                                                         int32_t* __restrict__ count_owned) {
    const int t = threadIdx.x;
    if (t >= count) return;
    const int id = ch.cell[t], slot = ch.slot[t];
    const int64_t at = (int64_t)(slot / max_boxes) * cells + id;
    const float r0 = g_rot[at * 2], r1 = g_rot[at * 2 + 1];
    const float rot = (float)atan2((double)r1, (double)r0);                                // :214
    const float cs = (float)cos((double)rot), sn = (float)sin((double)rot);
    const int c[3] = {id / (geo.Z * geo.Y), (id / geo.Z) % geo.Y, id % geo.Z};
    float* r = reinterpret_cast<float*>(recs + (int64_t)slot * INST_REC);
    for (int d = 0; d < 3; ++d) r[d] = geo.corner[d] + geo.res * (float)c[d];               // :206
    r[3] = cs;
    r[4] = sn;
    for (int d = 0; d < 3; ++d) r[5 + d] = g_scale[at * 3 + d];                             // :216
    recs[(int64_t)slot * INST_REC + 8] = (unsigned)ch.label[t];
    for (int d = 9; d < INST_REC; ++d) recs[(int64_t)slot * INST_REC + d] = 0u;
    if (count_in) count_in[slot] = 0;
    if (count_owned) count_owned[slot] = 0;
}

__global__ __launch_bounds__(256) void inst_assign(const float* __restrict__ pts, const float* __restrict__ prob, int64_t n,
                                                   const unsigned* __restrict__ recs, InstCats cats, int max_boxes,
                                                   float prob_thresh, int confident_only, int32_t* __restrict__ owner,
                                                   int32_t* __restrict__ count_in, int32_t* __restrict__ count_owned) {
    const int kc = blockIdx.y;
    const int nbox = cats.n_boxes[kc];
    recs += (int64_t)kc * max_boxes * INST_REC;
    const int64_t i = blockIdx.x * 256ll + threadIdx.x;
    const bool have = i < n;
    float p0 = 0, p1 = 0, p2 = 0;
    bool ok = have;                    // the point can be a member at all
    if (have) {
        p0 = pts[i * 3]; p1 = pts[i * 3 + 1]; p2 = pts[i * 3 + 2];
        if (confident_only) ok = prob[kc * n + i] > prob_thresh;                            // :245 (a NaN prob is not confident)
    }
    const bool counting = count_in != nullptr || count_owned != nullptr;
    __shared__ float4 l_rec[INST_GROUP * INST_REC / 4];
    // per-workgroup counts, flushed once per group: integer sums, the same for every arrival order
    __shared__ int l_in[INST_GROUP], l_owned[INST_GROUP];
    int own = -1;
    bool owned = false;
    for (int j0 = 0; j0 < nbox; j0 += INST_GROUP) {
        const int g = min(INST_GROUP, nbox - j0);
        // (the barrier frees the previous group's LDS; without counts a workgroup whose points all have their owner is done)
        if (counting) __syncthreads();
        else if (!__syncthreads_or(ok && !owned)) break;
        for (int e = threadIdx.x; e < g * INST_REC; e += 256)
            reinterpret_cast<unsigned*>(l_rec)[e] = recs[(int64_t)j0 * INST_REC + e];
        if (threadIdx.x < INST_GROUP) { l_in[threadIdx.x] = 0; l_owned[threadIdx.x] = 0; }
        __syncthreads();
        if (ok && (counting || !owned))
            for (int jj = 0; jj < g; ++jj) {
                const float4 a = l_rec[jj * 3], b = l_rec[jj * 3 + 1];
                const float sc[3] = {b.y, b.z, b.w};
                if (!inside_box(p0 - a.x, p1 - a.y, p2 - a.z, a.w, b.x, sc)) continue;       // :231-234
                if (count_in) atomicAdd(&l_in[jj], 1);
                if (!owned) {
                    owned = true;
                    own = __float_as_int(l_rec[jj * 3 + 2].x);
                    if (count_owned) atomicAdd(&l_owned[jj], 1);
                }
                if (!counting) break;
            }
        if (counting) {
            __syncthreads();
            if (threadIdx.x < g) {
                const int64_t slot = (int64_t)kc * max_boxes + j0 + threadIdx.x;
                if (count_in && l_in[threadIdx.x]) atomicAdd(&count_in[slot], l_in[threadIdx.x]);
                if (count_owned && l_owned[threadIdx.x]) atomicAdd(&count_owned[slot], l_owned[threadIdx.x]);
            }
        }
    }
    if (have) owner[kc * n + i] = own;
}

size_t inst_ws_bytes(int K, int max_boxes) {
    return cv_align_up((size_t)K * max_boxes * INST_REC * sizeof(unsigned), 256);
}

}  // namespace

extern "C" {

size_t cv_decode_instances_workspace_bytes(int num_cats, int max_boxes) {
    if (num_cats < 1 || num_cats > CV_MAX_CATEGORIES || max_boxes < 0 || (int64_t)num_cats * max_boxes >= (1ll << 31)) return 0;
    return inst_ws_bytes(num_cats, max_boxes);
}

int cv_decode_instances_f32(const float* d_grid_rot, const float* d_grid_scale, const int dims[3], const float h_corner3[3],
                            float res, const float* d_points, const float* d_prob, int64_t n, int num_cats,
                            const int64_t* h_cells, const int32_t* h_label_of, const int* h_n_boxes, int max_boxes,
                            float prob_thresh, int confident_only, int32_t* d_owner, int32_t* d_count_in,
                            int32_t* d_count_owned, void* d_ws, size_t ws_bytes, void* stream) {
    const int K = num_cats;
    CV_REQUIRE(K >= 1 && K <= CV_MAX_CATEGORIES, CV_EINVAL, "num_cats out of range (%d, 1..%d)", K, CV_MAX_CATEGORIES);
    CV_REQUIRE(d_grid_rot && d_grid_scale && dims && h_corner3 && d_points && d_owner && h_n_boxes, CV_EINVAL,
               "null pointer argument");
    CV_REQUIRE(d_prob || !confident_only, CV_EINVAL, "confident_only needs d_prob");
    CV_REQUIRE(n >= 0 && n <= (int64_t)0x7fffffff * 256, CV_EINVAL, "n out of range (%lld)", (long long)n);
    CV_REQUIRE(dims[0] > 0 && dims[1] > 0 && dims[2] > 0, CV_EINVAL, "bad grid dims");
    const int64_t G = (int64_t)dims[0] * dims[1] * dims[2];
    CV_REQUIRE(G < (1ll << 31), CV_EINVAL, "grid too large");
    CV_REQUIRE(max_boxes >= 0 && (int64_t)K * max_boxes < (1ll << 31), CV_EINVAL, "max_boxes out of range (%d)", max_boxes);
    int64_t total = 0;
    for (int k = 0; k < K; ++k) {
        CV_REQUIRE(h_n_boxes[k] >= 0 && h_n_boxes[k] <= max_boxes, CV_EINVAL, "n_boxes[%d] out of range (%d, 0..%d)", k,
                   h_n_boxes[k], max_boxes);
        total += h_n_boxes[k];
    }
    CV_REQUIRE(total == 0 || (h_cells && h_label_of), CV_EINVAL, "null pointer argument");
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < h_n_boxes[k]; ++j) {
            const int64_t cell = h_cells[(size_t)k * max_boxes + j];
            CV_REQUIRE(cell >= 0 && cell < G, CV_EINVAL, "cell %lld of category %d, box %d outside the grid (%lld cells)",
                       (long long)cell, k, j, (long long)G);
        }
    const size_t need = inst_ws_bytes(K, max_boxes);
    CV_REQUIRE(ws_bytes >= need && (d_ws || total == 0), CV_EINVAL, "workspace too small (%zu < %zu)", d_ws ? ws_bytes : (size_t)0,
               need);
    if (n == 0) return CV_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned* recs = static_cast<unsigned*>(d_ws);
    const Geo geo{dims[0], dims[1], dims[2], {h_corner3[0], h_corner3[1], h_corner3[2]}, res};
    InstChunk ch;
    InstCats cats;
    int fill = 0;
    for (int k = 0; k < CV_MAX_CATEGORIES; ++k) cats.n_boxes[k] = k < K ? h_n_boxes[k] : 0;
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < h_n_boxes[k]; ++j) {
            const size_t slot = (size_t)k * max_boxes + j;
            ch.cell[fill] = (int)h_cells[slot];
            ch.label[fill] = h_label_of[slot];
            ch.slot[fill] = (int)slot;
            if (++fill == INST_CHUNK) {
                inst_boxes<<<1, INST_CHUNK, 0, st>>>(d_grid_rot, d_grid_scale, geo, G, max_boxes, ch, fill, recs, d_count_in,
                                                     d_count_owned);
                CV_LAUNCH_CHECK();
                fill = 0;
            }
        }
    if (fill) {
        inst_boxes<<<1, INST_CHUNK, 0, st>>>(d_grid_rot, d_grid_scale, geo, G, max_boxes, ch, fill, recs, d_count_in, d_count_owned);
        CV_LAUNCH_CHECK();
    }
    inst_assign<<<dim3((unsigned)((n + 255) / 256), (unsigned)K), 256, 0, st>>>(d_points, d_prob, n, recs, cats, max_boxes,
                                                                                prob_thresh, confident_only, d_owner, d_count_in,
                                                                                d_count_owned);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

size_t cv_decode_workspace_bytes(const int dims[3], int64_t n, int max_iters) {
    if (!dims || max_iters <= 0) return 0;
    (void)n;
    return WsLayout((int64_t)dims[0] * dims[1] * dims[2], max_iters).total;
}

size_t cv_decode_scenes_workspace_bytes(const cv_decode_scene_job* jobs, int num_scenes, int max_iters) {
    if (!jobs || num_scenes < 1 || num_scenes > CV_MAX_SCENES) return 0;
    size_t total = 0;
    for (int b = 0; b < num_scenes; ++b) {
        const size_t one = cv_decode_workspace_bytes(jobs[b].dims, jobs[b].n, max_iters);
        if (one == 0) return 0;
        total += one;
    }
    return total;
}

int cv_decode_scenes_f32(const cv_decode_scene_job* jobs, int num_scenes, float res, const float* d_points, const float* d_xyz,
                         const float* d_prob, const int32_t* d_class, const cv_decode_params* params, int mutate_grid, void* d_ws,
                         size_t ws_bytes, int* h_n_cand, int64_t* h_cand_idx, int32_t* h_verdict, int* h_n_boxes, float* h_boxes,
                         float* h_scores, int32_t* h_classes, int* h_truncated, void* stream) {
    const DecodeCall c{nullptr, nullptr, nullptr, nullptr, nullptr, res, d_points, d_xyz, d_prob, d_class, 0, params,
                       mutate_grid, d_ws, ws_bytes, h_n_cand, h_cand_idx, h_verdict, h_n_boxes, h_boxes, h_scores, h_classes,
                       h_truncated, stream, nullptr};
    return cv_decode_scenes_run(c, jobs, num_scenes);
}

size_t cv_sizeof_decode_scene_job(void) { return sizeof(cv_decode_scene_job); }

size_t cv_decode_cat_workspace_bytes(const int dims[3], int64_t n, int max_iters, int num_cats) {
    if (num_cats < 1 || num_cats > CV_MAX_CATEGORIES) return 0;
    return (size_t)num_cats * cv_decode_workspace_bytes(dims, n, max_iters);
}

int cv_decode_f32(float* d_grid_obj, const float* d_grid_rot, const float* d_grid_scale,
                  const int dims[3], const float h_corner3[3], float res, const float* d_points,
                  const float* d_xyz, const float* d_prob, const int32_t* d_class, int64_t n,
                  const cv_decode_params* params, int mutate_grid, void* d_ws, size_t ws_bytes,
                  int* h_n_cand, int64_t* h_cand_idx, int32_t* h_verdict, int* h_n_boxes,
                  float* h_boxes, float* h_scores, int32_t* h_classes, int* h_truncated, void* stream) {
    const DecodeCall c{d_grid_obj, d_grid_rot, d_grid_scale, dims, h_corner3, res, d_points, d_xyz, d_prob, d_class, n, params,
                       mutate_grid, d_ws, ws_bytes, h_n_cand, h_cand_idx, h_verdict, h_n_boxes, h_boxes, h_scores, h_classes,
                       h_truncated, stream, nullptr};
    return cv_decode_run(c, 1, true);
}

int cv_decode_cat_f32(float* d_grid_obj, const float* d_grid_rot, const float* d_grid_scale, const int dims[3],
                      const float h_corner3[3], float res, const float* d_points, const float* d_xyz, const float* d_prob,
                      const int32_t* d_class, int64_t n, int num_cats, const cv_decode_params* params, int mutate_grid, void* d_ws,
                      size_t ws_bytes, int* h_n_cand, int64_t* h_cand_idx, int32_t* h_verdict, int* h_n_boxes, float* h_boxes,
                      float* h_scores, int32_t* h_classes, int* h_truncated, void* stream) {
    const DecodeCall c{d_grid_obj, d_grid_rot, d_grid_scale, dims, h_corner3, res, d_points, d_xyz, d_prob, d_class, n, params,
                       mutate_grid, d_ws, ws_bytes, h_n_cand, h_cand_idx, h_verdict, h_n_boxes, h_boxes, h_scores, h_classes,
                       h_truncated, stream, nullptr};
    return cv_decode_run(c, num_cats, false);
}

}  // extern "C"
