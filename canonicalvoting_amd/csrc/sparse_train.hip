// The backward of the sparse convolution for gfx950: the weight gradient (conv_wgrad, wgrad_reduce, the wgrad plan) and the
// transposed kernel map of the input gradient (transpose_map; the input gradient itself is a forward convolution,
// sparse_conv.hip), with their C entry points.  The row kernels of a training step - column sums, training-mode BatchNorm,
// copy_unless_flag - are row_ops.hip; sparse_conv_common.h holds what the sparse-convolution files share.
#include "cv_common.h"

#include <algorithm>

#include "sparse_conv_common.h"

using namespace cvsc;

namespace {

// ------------------------------------------------------------------ backward: weight gradient
// dW[j][ci][co] = sum_u x[nbr[u][j]][ci] * dy[u][co]   (the reduction runs over the output rows).
// One wave owns (offset j, 32 input channels, NB*32 output channels, a contiguous range of rows) and
// accumulates a 32 x NB*32 tile on the fp32 matrix cores: per MFMA step two rows u0,u1 are consumed -
// A operand lane l = x[nbr[u_{l>>5}][j]][ci0 + (l&31)], B operand lane l = dy[u_{l>>5}][co0 + nb*32 + (l&31)],
// both coalesced 128-byte row segments straight from L2.  Steps whose two rows both miss the neighbour
// are skipped (wave-uniform branch).  Partial tiles go to ws[split][K][cin][cout]; wgrad_reduce sums them.
// Launch plan of one weight-gradient call: offsets in heavy-first order (the centre offset pairs every row, face
// neighbours most, corners few - longest tasks are dispatched first) and a per-offset number of row splits so the
// tasks carry comparable numbers of pairs.  Partial tile of (offset j, split s) = slot first[j] + s.
constexpr int WG_MAX_K = 128;
struct WgradPlan {
    short order[WG_MAX_K];        // rank -> offset
    short nsplit[WG_MAX_K];       // by offset
    int first[WG_MAX_K];          // by offset: first partial slot
    int task_end[WG_MAX_K];       // by rank: cumulative (splits x ci blocks x co blocks)
};

// X6: the 16 rows of a step group are ONE K = 16 bf16 MFMA group: the eight values a lane holds for the steps t = 0..7
// (row 2t + half) are exactly its eight k slots (k = 8 * half + t, the same rows on the A and the B side), so the
// fp32 operands are split into bf16 triples in registers and six piece products replace eight fp32 MFMAs per nb
// (see conv_rows_wp; gradients keep the fp32 exponent range, which fp16 pairs would not).
// NA x NB blocks of 32 x 32 per wave: a wave that owns NA input-channel blocks reads each dy row segment once for all
// of them (and each x segment once for all NB output blocks).  With one input block per wave (the first version) a
// 96 -> 96 convolution moved 1536 bytes per (input, output) pair from L2 for three tiles - the kernel ran at the L2
// bandwidth (6.3 TB/s), not at the matrix rate; 3 x 3 blocks move 768 bytes for nine tiles.
template <int NA, int NB, int PIECES>      // PIECES 0: fp32 MFMA; 3: bf16 triples, six piece products; 1: operands rounded to bf16, one product
__global__ __launch_bounds__(THREADS, (NA * NB >= 8 ? 2 : 1)) void conv_wgrad(const float* __restrict__ x, int x_ld, int cin,
                                                      const float* __restrict__ dy, int dy_ld, int cout,
                                                      const int* __restrict__ nbr, int K, long long n_out,
                                                      WgradPlan plan, float* __restrict__ partial) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ci_blocks = (cin + NA * 32 - 1) / (NA * 32), co_blocks = (cout + NB * 32 - 1) / (NB * 32);
    int task = blockIdx.x * 4 + wave;
    if (task >= plan.task_end[K - 1]) return;
    int rank = 0;
    while (task >= plan.task_end[rank]) ++rank;                            // wave-uniform, K <= 128 entries
    if (rank) task -= plan.task_end[rank - 1];
    const int j = plan.order[rank], row_splits = plan.nsplit[j];
    const int split = task % row_splits; task /= row_splits;
    const int cob = task % co_blocks;
    const int cib = task / co_blocks;
    const long long r_lo = n_out * split / row_splits, r_hi = n_out * (split + 1) / row_splits;
    const int half = lane >> 5, l31 = lane & 31;
    const int ci0 = cib * NA * 32, co0 = cob * NB * 32;
    f32x16 acc[NA][NB];
#pragma unroll
    for (int na = 0; na < NA; ++na)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[na][nb][r] = 0.f;
    // 64 output rows per batch: every lane fetches one neighbour index (the next batch's is already in
    // flight), the rows that HAVE the neighbour are taken two at a time from the ballot mask (work
    // proportional to the existing pairs), and the operand loads of up to STEPS MFMA steps are issued back
    // to back before the matrix cores consume them.
    constexpr int STEPS = 8;
    auto fetch = [&](long long u0) -> int {
        const long long mu = u0 + lane;
        return mu < r_hi ? (nbr ? nbr[mu * K + j] : (int)mu) : -1;
    };
    int src_next = fetch(r_lo);
    for (long long u0 = r_lo; u0 < r_hi; u0 += 64) {
        const int src_l = src_next;
        src_next = fetch(u0 + 64);
        unsigned long long m = __ballot(src_l >= 0);
        while (m) {
            float av[STEPS][NA], bv[STEPS][NB];
            int nsteps = 0;
#pragma unroll
            for (int t = 0; t < STEPS; ++t) {
#pragma unroll
                for (int na = 0; na < NA; ++na) av[t][na] = 0.f;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) bv[t][nb] = 0.f;
                if (m) {                                                   // wave-uniform
                    const int ra = __ffsll((unsigned long long)m) - 1;
                    m &= m - 1;
                    int rb = -1;
                    if (m) { rb = __ffsll((unsigned long long)m) - 1; m &= m - 1; }
                    const int r = half ? rb : ra;                          // this half-wave's row of the pair
                    // shuffle with ALL lanes active: ds_bpermute returns 0 for an inactive source lane
                    const int got = __shfl(src_l, r >= 0 ? r : 0);
                    const int src = r >= 0 ? got : -1;
                    if (src >= 0) {
#pragma unroll
                        for (int na = 0; na < NA; ++na) {
                            const int ci = ci0 + na * 32 + l31;
                            if (ci < cin) av[t][na] = x[(long long)src * x_ld + ci];
                        }
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb) {
                            const int col = co0 + nb * 32 + l31;
                            if (col < cout) bv[t][nb] = dy[(u0 + r) * dy_ld + col];
                        }
                    }
                    nsteps = t + 1;
                }
            }
            if constexpr (PIECES == 1) {
                static_assert(STEPS == 8, "one bf16 MFMA group = 8 k slots per lane");
                bf16x8 a1[NA];
#pragma unroll
                for (int na = 0; na < NA; ++na)
                    a1[na] = __builtin_bit_cast(
                        bf16x8, make_uint4(cvt_pk_bf16(av[0][na], av[1][na]), cvt_pk_bf16(av[2][na], av[3][na]),
                                           cvt_pk_bf16(av[4][na], av[5][na]), cvt_pk_bf16(av[6][na], av[7][na])));
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const bf16x8 b1 = __builtin_bit_cast(
                        bf16x8, make_uint4(cvt_pk_bf16(bv[0][nb], bv[1][nb]), cvt_pk_bf16(bv[2][nb], bv[3][nb]),
                                           cvt_pk_bf16(bv[4][nb], bv[5][nb]), cvt_pk_bf16(bv[6][nb], bv[7][nb])));
#pragma unroll
                    for (int na = 0; na < NA; ++na)
                        acc[na][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[na], b1, acc[na][nb], 0, 0, 0);
                }
            } else if constexpr (PIECES == 3) {
                static_assert(STEPS == 8, "one bf16 MFMA group = 8 k slots per lane");
                bf16x8 a3[NA][3];
#pragma unroll
                for (int na = 0; na < NA; ++na) {
                    unsigned ap[3][4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) split3(av[2 * q][na], av[2 * q + 1][na], ap[0][q], ap[1][q], ap[2][q]);
#pragma unroll
                    for (int pc = 0; pc < 3; ++pc)
                        a3[na][pc] = __builtin_bit_cast(bf16x8, make_uint4(ap[pc][0], ap[pc][1], ap[pc][2], ap[pc][3]));
                }
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    unsigned bp[3][4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) split3(bv[2 * q][nb], bv[2 * q + 1][nb], bp[0][q], bp[1][q], bp[2][q]);
                    bf16x8 b3[3];
#pragma unroll
                    for (int pc = 0; pc < 3; ++pc)
                        b3[pc] = __builtin_bit_cast(bf16x8, make_uint4(bp[pc][0], bp[pc][1], bp[pc][2], bp[pc][3]));
#pragma unroll
                    for (int na = 0; na < NA; ++na) {
                        acc[na][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3[na][0], b3[2], acc[na][nb], 0, 0, 0);
                        acc[na][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3[na][2], b3[0], acc[na][nb], 0, 0, 0);
                        acc[na][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3[na][1], b3[1], acc[na][nb], 0, 0, 0);
                        acc[na][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3[na][0], b3[1], acc[na][nb], 0, 0, 0);
                        acc[na][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3[na][1], b3[0], acc[na][nb], 0, 0, 0);
                        acc[na][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3[na][0], b3[0], acc[na][nb], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < STEPS; ++t)
                    if (t < nsteps)
#pragma unroll
                        for (int na = 0; na < NA; ++na)
#pragma unroll
                            for (int nb = 0; nb < NB; ++nb)
                                acc[na][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t][na], bv[t][nb], acc[na][nb], 0, 0, 0);
            }
        }
    }
    float* p = partial + (long long)(plan.first[j] + split) * cin * cout;
#pragma unroll
    for (int na = 0; na < NA; ++na)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int col = co0 + nb * 32 + l31;
            if (col >= cout) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ci0 + na * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (ci < cin) p[(long long)ci * cout + col] = acc[na][nb][r];
            }
        }
}

// dW[j] = sum of offset j's partial tiles, in slot order (deterministic)
__global__ __launch_bounds__(256) void wgrad_reduce(const float* __restrict__ partial, int cc, int K, WgradPlan plan,
                                                    float* __restrict__ dw) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= (long long)cc * K) return;
    const int j = (int)(e / cc);
    const int w = (int)(e - (long long)j * cc);
    dw[e] = sum_in_order4(partial + (long long)plan.first[j] * cc + w, plan.nsplit[j], cc);
}

// transposed kernel map: nbr_t[i][j] = u with nbr[u][j] == i  (per offset the map is injective)
__global__ __launch_bounds__(256) void transpose_map(const int* __restrict__ nbr, long long n_out, int K,
                                                     int* __restrict__ nbr_t) {
    const long long t = blockIdx.x * 256ll + threadIdx.x;
    if (t >= n_out * K) return;
    const int i = nbr[t];
    if (i >= 0) nbr_t[(long long)i * K + (t % K)] = (int)(t / K);
}

}  // namespace

extern "C" {

constexpr long long WGRAD_TARGET_TASKS = 8192;

// ---- training support -------------------------------------------------------------------------
int cv_sp_transpose_map(const int32_t* d_nbr, long long n_out, int K, long long n_in, int32_t* d_nbr_t, void* stream) {
    CV_REQUIRE(d_nbr && d_nbr_t && n_out > 0 && n_in > 0 && K > 0, CV_EINVAL, "bad transpose_map arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CV_HIP_CHECK(hipMemsetAsync(d_nbr_t, 0xff, sizeof(int) * (size_t)n_in * K, st));
    transpose_map<<<(unsigned)((n_out * K + 255) / 256), 256, 0, st>>>(d_nbr, n_out, K, d_nbr_t);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

// Row splits of the weight-gradient reduction: enough (offset, ci block, co block, split) wave tasks to fill
// 256 CUs x 4 SIMDs a few times over even on the coarse levels (a few thousand rows), at least 128 rows each;
// the centre offset of an odd cubic kernel and its face neighbours hold the most pairs: they go first and get
// twice the splits (measured: profiles/wgrad_micro.py).
// input-channel blocks per wave (see conv_wgrad): as many as divide Cin / 32 while NA x NB accumulators fit
static int wgrad_na(int cin, int cout) {
    static const int na_max = getenv("CV_WGRAD_NA") ? atoi(getenv("CV_WGRAD_NA")) : 4;
    const int nb = nb_full(cout);
    int na = 1;
    if (cin % 32 == 0 && cin >= 64) {
        const int b = cin / 32;
        if (nb == 4) na = b % 2 == 0 ? 2 : 1;
        else if (nb == 3) na = b % 3 == 0 ? 3 : (b % 2 == 0 ? 2 : 1);
        else na = b % 4 == 0 ? 4 : (b % 2 == 0 ? 2 : (b % 3 == 0 ? 3 : 1));
    }
    return std::max(1, std::min(na, na_max));
}

static long long wgrad_plan(long long n_out, int cin, int cout, int K, WgradPlan* plan) {
    const int nb = nb_full(cout), na = wgrad_na(cin, cout);
    const int tiles = ((cin + na * 32 - 1) / (na * 32)) * ((cout + nb * 32 - 1) / (nb * 32));
    int ks = 1;
    while (ks * ks * ks < K) ++ks;
    const bool cubic = ks * ks * ks == K && (ks & 1) && ks > 1;
    int mult[WG_MAX_K], cls[WG_MAX_K], msum = 0;
    for (int j = 0; j < K; ++j) {
        int d1 = 3;
        if (cubic) {
            const int h = ks / 2;
            d1 = std::abs(j % ks - h) + std::abs(j / ks % ks - h) + std::abs(j / (ks * ks) - h);
        }
        // splits per offset class (centre / face / edge+corner of an odd cubic kernel); CV_WGRAD_MULT="c,f,o" overrides (experiment)
        static int m_c = 2, m_f = 2, m_o = 1;
        static const bool m_env = [] {
            const char* e = getenv("CV_WGRAD_MULT");
            if (e) sscanf(e, "%d,%d,%d", &m_c, &m_f, &m_o);
            m_c = std::max(1, m_c); m_f = std::max(1, m_f); m_o = std::max(1, m_o);      // msum divides below
            return true;
        }();
        (void)m_env;
        mult[j] = !cubic ? 1 : d1 == 0 ? m_c : d1 == 1 ? m_f : m_o;
        cls[j] = !cubic ? 2 : d1 == 0 ? 0 : d1 == 1 ? 1 : 2;
        msum += mult[j];
    }
    static const long long target_tasks = std::max(1ll, getenv("CV_WGRAD_TASKS") ? atoll(getenv("CV_WGRAD_TASKS")) : WGRAD_TARGET_TASKS);
    static const long long cap_env = std::max(1ll, getenv("CV_WGRAD_CAP") ? atoll(getenv("CV_WGRAD_CAP")) : 64);
    const long long want = (target_tasks + (long long)msum * tiles - 1) / ((long long)msum * tiles);
    // partial tiles <= 96 MB (they are written once and read once by wgrad_reduce); few-offset kernels (1x1, 2x2x2)
    // have few (offset, block) tasks and get their parallelism from the rows instead: up to 1024 row splits
    const long long ws_cap = (96ll << 20) / ((long long)msum * cin * cout * 4);
    const long long cap = K <= 8 ? 1024 : cap_env;
    const long long base = std::max<long long>(1, std::min({cap, want, n_out / (K <= 8 ? 128 : 256), ws_cap}));
    long long slots = 0;
    int rank = 0, tasks = 0;
    for (int pass = 0; pass < 3; ++pass)
        for (int j = 0; j < K; ++j) {
            if (cls[j] != pass) continue;
            const int sp = (int)std::max<long long>(1, std::min<long long>(base * mult[j], n_out / 128));
            if (plan) {
                plan->order[rank] = (short)j;
                plan->nsplit[j] = (short)sp;
                plan->first[j] = (int)slots;
                tasks += sp * tiles;
                plan->task_end[rank] = tasks;
            }
            slots += sp;
            ++rank;
        }
    return slots;
}

size_t cv_sp_wgrad_workspace_bytes(long long n_out, int cin, int cout, int K) {
    if (n_out <= 0 || cin <= 0 || cout <= 0 || K <= 0 || K > WG_MAX_K) return 0;
    return 256 + sizeof(float) * (size_t)wgrad_plan(n_out, cin, cout, K, nullptr) * (size_t)cin * cout;
}

int cv_sp_conv_wgrad_px_f32(const float* d_x, int x_ld, int cin, const float* d_dy, int dy_ld, int cout,
                            const int32_t* d_nbr, int K, long long n_out, float* d_dw, void* d_ws, size_t ws_bytes,
                            int pieces, void* stream) {
    CV_REQUIRE(d_x && d_dy && d_dw && d_ws, CV_EINVAL, "null pointer argument");
    CV_REQUIRE(n_out > 0 && cin > 0 && cout > 0 && K > 0 && x_ld >= cin && dy_ld >= cout, CV_EINVAL, "bad wgrad sizes");
    CV_REQUIRE(K <= WG_MAX_K, CV_EINVAL, "kernel volume above 128 is not supported");
    CV_REQUIRE(d_nbr || K == 1, CV_EINVAL, "a kernel map is required unless K == 1");
    CV_REQUIRE(ws_bytes >= cv_sp_wgrad_workspace_bytes(n_out, cin, cout, K), CV_ENOMEM, "workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    WgradPlan plan = {};
    wgrad_plan(n_out, cin, cout, K, &plan);
    float* partial = static_cast<float*>(d_ws);
    // any Cin: channels beyond Cin are zero lanes of the 32-wide A operand (stem: Cin = 3)
    const unsigned grid = (unsigned)((plan.task_end[K - 1] + 3) / 4);
    CV_REQUIRE(pieces == 0 || pieces == 1 || pieces == 3, CV_EINVAL,
               "pieces is 0 (fp32 MFMA), 3 (six bf16 piece products per fp32 product) or 1 (one bf16 product)");
#define CV_WGRAD_LAUNCH(NAV, NBV)                                                                                    \
    do {                                                                                                             \
        if (pieces == 3) conv_wgrad<NAV, NBV, 3><<<grid, THREADS, 0, st>>>(d_x, x_ld, cin, d_dy, dy_ld, cout, d_nbr, K, n_out, plan, partial); \
        else if (pieces == 1) conv_wgrad<NAV, NBV, 1><<<grid, THREADS, 0, st>>>(d_x, x_ld, cin, d_dy, dy_ld, cout, d_nbr, K, n_out, plan, partial); \
        else conv_wgrad<NAV, NBV, 0><<<grid, THREADS, 0, st>>>(d_x, x_ld, cin, d_dy, dy_ld, cout, d_nbr, K, n_out, plan, partial);   \
    } while (0)
    const int na = wgrad_na(cin, cout);
    switch (nb_full(cout) * 10 + na) {
        case 11: CV_WGRAD_LAUNCH(1, 1); break;
        case 12: CV_WGRAD_LAUNCH(2, 1); break;
        case 13: CV_WGRAD_LAUNCH(3, 1); break;
        case 14: CV_WGRAD_LAUNCH(4, 1); break;
        case 21: CV_WGRAD_LAUNCH(1, 2); break;
        case 22: CV_WGRAD_LAUNCH(2, 2); break;
        case 23: CV_WGRAD_LAUNCH(3, 2); break;
        case 24: CV_WGRAD_LAUNCH(4, 2); break;
        case 31: CV_WGRAD_LAUNCH(1, 3); break;
        case 32: CV_WGRAD_LAUNCH(2, 3); break;
        case 33: CV_WGRAD_LAUNCH(3, 3); break;
        case 41: CV_WGRAD_LAUNCH(1, 4); break;
        case 42: CV_WGRAD_LAUNCH(2, 4); break;
        default: CV_REQUIRE(false, CV_EINVAL, "no weight-gradient kernel for this block shape");
    }
#undef CV_WGRAD_LAUNCH
    CV_LAUNCH_CHECK();
    const long long per = (long long)K * cin * cout;
    wgrad_reduce<<<(unsigned)((per + 255) / 256), 256, 0, st>>>(partial, cin * cout, K, plan, d_dw);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_sp_conv_wgrad_f32(const float* d_x, int x_ld, int cin, const float* d_dy, int dy_ld, int cout,
                         const int32_t* d_nbr, int K, long long n_out, float* d_dw, void* d_ws, size_t ws_bytes,
                         void* stream) {
    // CV_WGRAD_X6=0: exact fp32 products on v_mfma_f32_32x32x2_f32 instead of six bf16 piece products
    static const bool x6 = !(getenv("CV_WGRAD_X6") && atoi(getenv("CV_WGRAD_X6")) == 0);
    return cv_sp_conv_wgrad_px_f32(d_x, x_ld, cin, d_dy, dy_ld, cout, d_nbr, K, n_out, d_dw, d_ws, ws_bytes,
                                   x6 ? 3 : 0, stream);
}

}  // extern "C"
