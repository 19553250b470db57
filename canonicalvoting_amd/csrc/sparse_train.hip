// The training side of the sparse convolution for gfx950: what the eval path never launches.
//   weight gradient (conv_wgrad, wgrad_reduce) and the transposed kernel map of the input gradient (transpose_map; the input
//   gradient itself is a forward convolution, sparse_conv.hip), column sums (the bias gradient), BatchNorm in training mode
//   (batch statistics, backward) and the guarded copy of an optimiser step (copy_unless_flag), with their C entry points.
// The forward kernels, the weight packers, the mask orders, the elementwise / hl helpers, bn_fold, the heads and the
// dispatcher are in sparse_conv.hip; sparse_conv_common.h holds what both files use.
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
    const float* p = partial + (long long)plan.first[j] * cc + w;
    // four interleaved running sums (slots k % 4), combined in a fixed order: four independent load chains in flight
    const int ns = plan.nsplit[j];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int k = 0;
    for (; k + 3 < ns; k += 4) {
        s0 += p[(long long)k * cc];
        s1 += p[(long long)(k + 1) * cc];
        s2 += p[(long long)(k + 2) * cc];
        s3 += p[(long long)(k + 3) * cc];
    }
    for (; k < ns; ++k) s0 += p[(long long)k * cc];
    dw[e] = (s0 + s1) + (s2 + s3);
}

// transposed kernel map: nbr_t[i][j] = u with nbr[u][j] == i  (per offset the map is injective)
__global__ __launch_bounds__(256) void transpose_map(const int* __restrict__ nbr, long long n_out, int K,
                                                     int* __restrict__ nbr_t) {
    const long long t = blockIdx.x * 256ll + threadIdx.x;
    if (t >= n_out * K) return;
    const int i = nbr[t];
    if (i >= 0) nbr_t[(long long)i * K + (t % K)] = (int)(t / K);
}

// column sums (bias gradient): blocks over (32 columns, row chunk); partial sums meet through fp32
// atomics on the c output words (out is pre-zeroed)
__global__ __launch_bounds__(256) void col_sum(const float* __restrict__ x, long long n, int c, int ld,
                                               float* __restrict__ out) {
    __shared__ float s[8][32];
    const int col = blockIdx.x * 32 + (threadIdx.x & 31), ry = threadIdx.x >> 5;
    const long long r_lo = n * blockIdx.y / gridDim.y, r_hi = n * (blockIdx.y + 1) / gridDim.y;
    float acc = 0.f;
    if (col < c)
        for (long long r = r_lo + ry; r < r_hi; r += 8) acc += x[r * ld + col];
    s[ry][threadIdx.x & 31] = acc;
    __syncthreads();
    if (ry == 0 && col < c) {
        float t = 0.f;
        for (int k = 0; k < 8; ++k) t += s[k][threadIdx.x & 31];
        unsafeAtomicAdd(&out[col], t);
    }
}

// the same sums without atomics: every (32 columns, row chunk) block writes its partial sums to ws[chunk][c], a second
// launch adds the chunks of a column in chunk order - the result does not depend on the order in which workgroups run
__global__ __launch_bounds__(256) void col_sum_partial(const float* __restrict__ x, long long n, int c, int ld,
                                                       float* __restrict__ ws) {
    __shared__ float s[8][32];
    const int col = blockIdx.x * 32 + (threadIdx.x & 31), ry = threadIdx.x >> 5;
    const long long r_lo = n * blockIdx.y / gridDim.y, r_hi = n * (blockIdx.y + 1) / gridDim.y;
    float acc = 0.f;
    if (col < c)
        for (long long r = r_lo + ry; r < r_hi; r += 8) acc += x[r * ld + col];
    s[ry][threadIdx.x & 31] = acc;
    __syncthreads();
    if (ry == 0 && col < c) {
        float t = 0.f;
        for (int k = 0; k < 8; ++k) t += s[k][threadIdx.x & 31];
        ws[(long long)blockIdx.y * c + col] = t;
    }
}
__global__ __launch_bounds__(256) void col_sum_chunks(const float* __restrict__ ws, int chunks, int c,
                                                      float* __restrict__ out) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= c) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;          // four load chains, combined in a fixed order
    int k = 0;
    for (; k + 3 < chunks; k += 4) {
        s0 += ws[(long long)k * c + col];
        s1 += ws[(long long)(k + 1) * c + col];
        s2 += ws[(long long)(k + 2) * c + col];
        s3 += ws[(long long)(k + 3) * c + col];
    }
    for (; k < chunks; ++k) s0 += ws[(long long)k * c + col];
    out[col] = (s0 + s1) + (s2 + s3);
}

// ------------------------------------------------------------------ BatchNorm in training mode
// MinkowskiBatchNorm = nn.BatchNorm1d over the [N, C] feature rows (utils/minkunet.py:56): batch mean and
// biased variance per channel.  Two-level column reduction: blocks of (32 channels x 8 row lanes) over row
// chunks accumulate in double, a second tiny kernel combines the chunks.
constexpr int BN_CHUNKS = 1024;

template <int MODE>   // 0: sum x, sum x^2      1: sum dy', sum dy'*xhat   (dy' = dy masked by y > 0 if y given)
__global__ __launch_bounds__(256) void bn_col_reduce(const float* __restrict__ x, const float* __restrict__ dy,
                                                     const float* __restrict__ y, long long n, int c, int ld,
                                                     const float* __restrict__ mean, const float* __restrict__ var,
                                                     float eps, double* __restrict__ partial) {
    __shared__ double s0[8][32], s1[8][32];
    const int col = blockIdx.x * 32 + (threadIdx.x & 31), ry = threadIdx.x >> 5;
    const long long r_lo = n * blockIdx.y / gridDim.y, r_hi = n * (blockIdx.y + 1) / gridDim.y;
    double a0 = 0.0, a1 = 0.0;
    if (col < c) {
        float mu = 0.f, istd = 0.f;
        if (MODE == 1) { mu = mean[col]; istd = 1.0f / sqrtf(var[col] + eps); }
        for (long long r = r_lo + ry; r < r_hi; r += 8) {
            const float xv = x[r * ld + col];
            if (MODE == 0) { a0 += (double)xv; a1 += (double)xv * (double)xv; }
            else {
                float g = dy[r * ld + col];
                if (y && !(y[r * ld + col] > 0.f)) g = 0.f;
                a0 += (double)g;
                a1 += (double)(g * ((xv - mu) * istd));
            }
        }
    }
    s0[ry][threadIdx.x & 31] = a0; s1[ry][threadIdx.x & 31] = a1;
    __syncthreads();
    if (ry == 0 && col < c) {
        double t0 = 0.0, t1 = 0.0;
        for (int k = 0; k < 8; ++k) { t0 += s0[k][threadIdx.x & 31]; t1 += s1[k][threadIdx.x & 31]; }
        partial[((long long)blockIdx.y * c + col) * 2 + 0] = t0;
        partial[((long long)blockIdx.y * c + col) * 2 + 1] = t1;
    }
}

// float4 flavour of bn_col_reduce (c % 4 == 0, c <= 1024, ld % 4 == 0, 16-byte aligned): a thread owns a quad of
// channels, 256 / (c/4) row lanes per block, four rows of loads in flight per thread; the scalar kernel above kept
// one 4-byte load per thread in flight (1.8 TB/s on the ts1 levels).  Same partial layout, fixed summation order.
// The ReLU mask of a BatchNorm + ReLU output for its backward: either the output rows themselves (y > 0) or one bit per
// element, [row][c / 32] words written by the forward pass (cv_sp_affine_hl_f32) - a 32nd of the bytes of y in the two
// backward passes that only want to know where the ReLU was open.
__device__ __forceinline__ float4 relu_open4(const float* __restrict__ y, const unsigned* __restrict__ ybits, long long r, int k,
                                             int ld, int c) {
    if (ybits) {
        const unsigned w = ybits[r * (c >> 5) + (k >> 5)] >> (k & 31);
        return make_float4((float)(w & 1u), (float)((w >> 1) & 1u), (float)((w >> 2) & 1u), (float)((w >> 3) & 1u));
    }
    return *reinterpret_cast<const float4*>(y + r * ld + k);
}
template <int MODE>
__global__ __launch_bounds__(256) void bn_col_reduce4(const float* __restrict__ x, const float* __restrict__ dy,
                                                      const float* __restrict__ y, long long n, int c, int ld,
                                                      const float* __restrict__ mean, const float* __restrict__ var,
                                                      float eps, double* __restrict__ partial,
                                                      const unsigned* __restrict__ ybits = nullptr) {
    __shared__ double red[256][9];                     // [thread][2 x 4 sums], padded
    const int cq = c >> 2, rl = 256 / cq;              // row lanes
    const int quad = threadIdx.x % cq, lane_r = threadIdx.x / cq;
    const long long r_lo = n * blockIdx.x / gridDim.x, r_hi = n * (blockIdx.x + 1) / gridDim.x;
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (lane_r < rl) {
        const int k = quad * 4;
        float4 mu = make_float4(0.f, 0.f, 0.f, 0.f), is = mu;
        if (MODE == 1) {
            mu = *reinterpret_cast<const float4*>(mean + k);
            const float4 v = *reinterpret_cast<const float4*>(var + k);
            is = make_float4(1.0f / sqrtf(v.x + eps), 1.0f / sqrtf(v.y + eps), 1.0f / sqrtf(v.z + eps), 1.0f / sqrtf(v.w + eps));
        }
        auto take = [&](const float4& xv, float4 g, const float4& yv, bool has_y) {
            if (MODE == 0) {
                a[0] += (double)xv.x; a[1] += (double)xv.y; a[2] += (double)xv.z; a[3] += (double)xv.w;
                a[4] += (double)xv.x * (double)xv.x; a[5] += (double)xv.y * (double)xv.y;
                a[6] += (double)xv.z * (double)xv.z; a[7] += (double)xv.w * (double)xv.w;
            } else {
                if (has_y) {
                    if (!(yv.x > 0.f)) g.x = 0.f;
                    if (!(yv.y > 0.f)) g.y = 0.f;
                    if (!(yv.z > 0.f)) g.z = 0.f;
                    if (!(yv.w > 0.f)) g.w = 0.f;
                }
                a[0] += (double)g.x; a[1] += (double)g.y; a[2] += (double)g.z; a[3] += (double)g.w;
                a[4] += (double)(g.x * ((xv.x - mu.x) * is.x)); a[5] += (double)(g.y * ((xv.y - mu.y) * is.y));
                a[6] += (double)(g.z * ((xv.z - mu.z) * is.z)); a[7] += (double)(g.w * ((xv.w - mu.w) * is.w));
            }
        };
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        long long r = r_lo + lane_r;
        for (; r + 3ll * rl < r_hi; r += 4ll * rl) {
            float4 xv[4], gv[4], yv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long o = (r + (long long)u * rl) * ld + k;
                xv[u] = *reinterpret_cast<const float4*>(x + o);
                gv[u] = MODE == 1 ? *reinterpret_cast<const float4*>(dy + o) : z4;
                yv[u] = (MODE == 1 && (y || ybits)) ? relu_open4(y, ybits, r + (long long)u * rl, k, ld, c) : z4;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) take(xv[u], gv[u], yv[u], y != nullptr || ybits != nullptr);
        }
        for (; r < r_hi; r += rl) {
            const long long o = r * ld + k;
            take(*reinterpret_cast<const float4*>(x + o), MODE == 1 ? *reinterpret_cast<const float4*>(dy + o) : z4,
                 (MODE == 1 && (y || ybits)) ? relu_open4(y, ybits, r, k, ld, c) : z4, y != nullptr || ybits != nullptr);
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) red[threadIdx.x][i] = a[i];
    __syncthreads();
    if (threadIdx.x < cq) {
        double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int q = 0; q < rl; ++q)
#pragma unroll
            for (int i = 0; i < 8; ++i) t[i] += red[q * cq + threadIdx.x][i];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            partial[((long long)blockIdx.x * c + threadIdx.x * 4 + i) * 2 + 0] = t[i];
            partial[((long long)blockIdx.x * c + threadIdx.x * 4 + i) * 2 + 1] = t[4 + i];
        }
    }
}

// MODE 0: mean/var from the partials, running statistics update (momentum, unbiased variance), folded
// scale/shift for the apply pass.  MODE 1: out0 = sum dy' (d beta), out1 = sum dy'*xhat (d gamma).
// 16 lanes per channel: each sums every 16th chunk (independent loads in flight instead of one thread walking 256
// dependent ones: 23 -> a few us per call, 124 calls per training step), then a fixed-order butterfly.
template <int MODE>
__global__ __launch_bounds__(256) void bn_col_finish(const double* __restrict__ partial, int chunks, long long n, int c,
                                                     float* out0, float* out1, float* running_mean, float* running_var,
                                                     float momentum, const float* gamma, const float* beta, float eps,
                                                     float* scale, float* shift) {
    const int sub = threadIdx.x & 15;
    const int k = blockIdx.x * 16 + (threadIdx.x >> 4);
    double t0 = 0.0, t1 = 0.0;
    if (k < c)
        for (int q = sub; q < chunks; q += 16) {
            t0 += partial[((long long)q * c + k) * 2];
            t1 += partial[((long long)q * c + k) * 2 + 1];
        }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
        t0 += __shfl_xor(t0, off);
        t1 += __shfl_xor(t1, off);
    }
    if (k >= c || sub != 0) return;
    if (MODE == 0) {
        const double mu = t0 / (double)n;
        double v = t1 / (double)n - mu * mu;
        if (v < 0.0) v = 0.0;
        out0[k] = (float)mu;
        out1[k] = (float)v;
        if (running_mean) {
            const double unb = n > 1 ? v * (double)n / (double)(n - 1) : v;
            running_mean[k] = (1.f - momentum) * running_mean[k] + momentum * (float)mu;
            running_var[k] = (1.f - momentum) * running_var[k] + momentum * (float)unb;
        }
        const float sc = gamma[k] / sqrtf((float)v + eps);
        scale[k] = sc;
        shift[k] = beta[k] - (float)mu * sc;
    } else {
        out0[k] = (float)t0;
        out1[k] = (float)t1;
    }
}

constexpr int BN_SLOT_BLOCKS = 4096;          // = the grid cap of the launch with the hl twin (cv_sp_bn_backward_hl_f32: CV_BN_SLOT_WORDS)
// dx = gamma*istd * (dy' - sum_dy/n - xhat * sum_dy_xhat/n)
__global__ __launch_bounds__(256) void bn_backward_apply(const float* __restrict__ x, const float* __restrict__ dy,
                                                         const float* __restrict__ y, long long n, int c, int ld,
                                                         const float* __restrict__ mean, const float* __restrict__ var,
                                                         float eps, const float* __restrict__ gamma,
                                                         const float* __restrict__ sum_dy,
                                                         const float* __restrict__ sum_dy_xhat, float* __restrict__ dx,
                                                         float* __restrict__ dres) {
    const float inv_n = 1.0f / (float)n;
    for (long long t = blockIdx.x * 256ll + threadIdx.x; t < n * c; t += (long long)gridDim.x * 256) {
        const long long r = t / c;
        const int k = (int)(t - r * c);
        const float istd = 1.0f / sqrtf(var[k] + eps);
        const float xh = (x[r * ld + k] - mean[k]) * istd;
        float g = dy[r * ld + k];
        if (y && !(y[r * ld + k] > 0.f)) g = 0.f;
        dx[r * ld + k] = gamma[k] * istd * (g - sum_dy[k] * inv_n - xh * sum_dy_xhat[k] * inv_n);
        if (dres) dres[r * ld + k] = g;
    }
}

// float4 flavour (c, ld % 4 == 0, 16-byte aligned)
__global__ __launch_bounds__(256) void bn_backward_apply4(const float* __restrict__ x, const float* __restrict__ dy,
                                                          const float* __restrict__ y, long long n, int c, int ld,
                                                          const float* __restrict__ mean, const float* __restrict__ var,
                                                          float eps, const float* __restrict__ gamma,
                                                          const float* __restrict__ sum_dy,
                                                          const float* __restrict__ sum_dy_xhat, float* __restrict__ dx,
                                                          float* __restrict__ dres, float* __restrict__ dx_hl = nullptr,
                                                          unsigned* __restrict__ slot = nullptr,
                                                          int* __restrict__ range_flag = nullptr,
                                                          const unsigned* __restrict__ ybits = nullptr) {
    const float inv_n = 1.0f / (float)n;
    const int cq = c >> 2;
    // dx_hl: dx once more as fp16 pairs for the input-gradient convolution of the layer below, times the power of two that put
    // the PREVIOUS step's largest |dx| of this layer into [2^9, 2^10) (a factor of 64 to the fp16 range - beyond it the range
    // flag stops the optimizer step).  slot: BN_SLOT_BLOCKS words, one per workgroup, that receive this step's maxima (bits of
    // non-negative floats; plain stores - atomics on shared words cost ~1 us each across the XCDs: a fixed 28-50 us per launch),
    // BN_SLOT_BLOCKS words with the previous step's, one float that receives the inverse factor for that convolution's epilogue.
    __shared__ unsigned wred[4];
    float hs = 1.f, dmax = 0.f;
    if (dx_hl) {
        unsigned mb = 0u;
        for (int i = threadIdx.x; i < BN_SLOT_BLOCKS; i += 256) mb = max(mb, slot[BN_SLOT_BLOCKS + i]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mb = max(mb, (unsigned)__shfl_xor((int)mb, off));
        if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = mb;
        __syncthreads();
        mb = max(max(wred[0], wred[1]), max(wred[2], wred[3]));
        __syncthreads();
        const unsigned E = (mb >> 23) & 255u;        // m in [2^(E - 127), 2^(E - 126))
        hs = (E >= 10u && E <= 250u) ? __uint_as_float((263u - E) << 23) : 1.f;          // 2^(136 - E)
        if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<float*>(slot)[2 * BN_SLOT_BLOCKS] = 1.f / hs;
    }
    for (long long t = blockIdx.x * 256ll + threadIdx.x; t < n * cq; t += (long long)gridDim.x * 256) {
        const long long r = t / cq;
        const int k = (int)(t - r * cq) * 4;
        const long long o = r * ld + k;
        const float4 xv = *reinterpret_cast<const float4*>(x + o);
        float4 g = *reinterpret_cast<const float4*>(dy + o);
        if (y || ybits) {
            const float4 yv = relu_open4(y, ybits, r, k, ld, c);
            if (!(yv.x > 0.f)) g.x = 0.f;
            if (!(yv.y > 0.f)) g.y = 0.f;
            if (!(yv.z > 0.f)) g.z = 0.f;
            if (!(yv.w > 0.f)) g.w = 0.f;
        }
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, gs[4] = {g.x, g.y, g.z, g.w};
        float d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float istd = 1.0f / sqrtf(var[k + i] + eps);
            const float xh = (xs[i] - mean[k + i]) * istd;
            d[i] = gamma[k + i] * istd * (gs[i] - sum_dy[k + i] * inv_n - xh * sum_dy_xhat[k + i] * inv_n);
        }
        *reinterpret_cast<float4*>(dx + o) = make_float4(d[0], d[1], d[2], d[3]);
        if (dres) *reinterpret_cast<float4*>(dres + o) = g;
        if (dx_hl) {
            dmax = fmaxf(fmaxf(dmax, fmaxf(fabsf(d[0]), fabsf(d[1]))), fmaxf(fabsf(d[2]), fabsf(d[3])));
            const float4 v = make_float4(d[0] * hs, d[1] * hs, d[2] * hs, d[3] * hs);
            if (range_flag && hl_out_of_range(v)) *range_flag = 1;
            hl_store4(dx_hl + r * ld, k, v);
        }
    }
    if (dx_hl) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, off));
        if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = __float_as_uint(dmax);
        __syncthreads();
        if (threadIdx.x == 0) slot[blockIdx.x] = max(max(wred[0], wred[1]), max(wred[2], wred[3]));
    }
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

int cv_sp_col_sum_f32(const float* d_x, long long n, int c, int ld, float* d_out, void* stream) {
    CV_REQUIRE(d_x && d_out && n > 0 && c > 0 && ld >= c, CV_EINVAL, "bad col_sum arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CV_HIP_CHECK(hipMemsetAsync(d_out, 0, sizeof(float) * c, st));
    dim3 grid((unsigned)((c + 31) / 32), (unsigned)std::min<long long>(256, (n + 1023) / 1024));
    col_sum<<<grid, 256, 0, st>>>(d_x, n, c, ld, d_out);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

static unsigned col_sum_chunks_for(long long n) { return (unsigned)std::min<long long>(256, (n + 1023) / 1024); }

size_t cv_sp_col_sum_workspace_bytes(long long n, int c) {
    if (n <= 0 || c <= 0) return 0;
    return sizeof(float) * (size_t)col_sum_chunks_for(n) * (size_t)c;
}

int cv_sp_col_sum_det_f32(const float* d_x, long long n, int c, int ld, float* d_out, void* d_ws, size_t ws_bytes,
                          void* stream) {
    CV_REQUIRE(d_x && d_out && d_ws && n > 0 && c > 0 && ld >= c, CV_EINVAL, "bad col_sum arguments");
    CV_REQUIRE(ws_bytes >= cv_sp_col_sum_workspace_bytes(n, c), CV_ENOMEM, "workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned chunks = col_sum_chunks_for(n);
    float* ws = static_cast<float*>(d_ws);
    col_sum_partial<<<dim3((unsigned)((c + 31) / 32), chunks), 256, 0, st>>>(d_x, n, c, ld, ws);
    CV_LAUNCH_CHECK();
    col_sum_chunks<<<(unsigned)((c + 255) / 256), 256, 0, st>>>(ws, (int)chunks, c, d_out);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

// dst_i = src_i for up to COPY_BATCH small tensors in ONE launch, unless *flag != 0 (cv_sp_copy_unless_flag)
constexpr int COPY_BATCH = 96;
struct CopyJobs {
    const uint32_t* src[COPY_BATCH];
    uint32_t* dst[COPY_BATCH];
    int words[COPY_BATCH];
};
static __global__ __launch_bounds__(256) void copy_unless_flag(CopyJobs jobs, const int32_t* __restrict__ flag) {
    if (flag && __builtin_nontemporal_load(flag) != 0) return;
    const uint32_t* s = jobs.src[blockIdx.x];
    uint32_t* d = jobs.dst[blockIdx.x];
    for (int i = threadIdx.x; i < jobs.words[blockIdx.x]; i += 256) d[i] = s[i];
}

int cv_sp_copy_unless_flag(const void* const* h_src, void* const* h_dst, const long long* h_bytes, int n, const int32_t* flag,
                           void* stream) {
    CV_REQUIRE(n >= 0 && (n == 0 || (h_src && h_dst && h_bytes)), CV_EINVAL, "bad copy batch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int base = 0; base < n; base += COPY_BATCH) {
        CopyJobs jobs;
        const int m = std::min(COPY_BATCH, n - base);
        for (int i = 0; i < m; ++i) {
            CV_REQUIRE(h_src[base + i] && h_dst[base + i] && h_bytes[base + i] >= 0 && h_bytes[base + i] % 4 == 0 &&
                           h_bytes[base + i] < (1ll << 33), CV_EINVAL, "copy %d: null pointer or a size that is not a multiple of 4 bytes", base + i);
            jobs.src[i] = static_cast<const uint32_t*>(h_src[base + i]);
            jobs.dst[i] = static_cast<uint32_t*>(h_dst[base + i]);
            jobs.words[i] = (int)(h_bytes[base + i] / 4);
        }
        copy_unless_flag<<<m, 256, 0, st>>>(jobs, flag);
        CV_LAUNCH_CHECK();
    }
    return CV_OK;
}

size_t cv_sp_bn_workspace_bytes(int c) { return c > 0 ? 256 + sizeof(double) * 2 * (size_t)BN_CHUNKS * c : 0; }

static int bn_chunks(long long n) { return (int)std::min<long long>(BN_CHUNKS, std::max<long long>(1, n / 256)); }

// Training-mode BatchNorm statistics of x[n][c]: d_mean, d_var (biased), running statistics updated in place
// (may be NULL), and the folded d_scale/d_shift for cv_sp_affine_f32 (y = x*scale + shift).
int cv_sp_bn_stats_f32(const float* d_x, long long n, int c, int ld, const float* d_gamma, const float* d_beta,
                       float eps, float momentum, float* d_running_mean, float* d_running_var, float* d_mean,
                       float* d_var, float* d_scale, float* d_shift, void* d_ws, size_t ws_bytes, void* stream) {
    CV_REQUIRE(d_x && d_gamma && d_beta && d_mean && d_var && d_scale && d_shift && d_ws, CV_EINVAL, "null pointer argument");
    CV_REQUIRE(n > 0 && c > 0 && ld >= c, CV_EINVAL, "bad bn sizes");
    CV_REQUIRE(ws_bytes >= cv_sp_bn_workspace_bytes(c), CV_ENOMEM, "workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(d_ws);
    const int chunks = bn_chunks(n);
    dim3 grid((unsigned)((c + 31) / 32), (unsigned)chunks);
    if (c % 4 == 0 && c <= 1024 && ld % 4 == 0 && aligned16(d_x))
        bn_col_reduce4<0><<<chunks, 256, 0, st>>>(d_x, nullptr, nullptr, n, c, ld, nullptr, nullptr, eps, partial);
    else
        bn_col_reduce<0><<<grid, 256, 0, st>>>(d_x, nullptr, nullptr, n, c, ld, nullptr, nullptr, eps, partial);
    CV_LAUNCH_CHECK();
    bn_col_finish<0><<<(c + 15) / 16, 256, 0, st>>>(partial, chunks, n, c, d_mean, d_var, d_running_mean,
                                                     d_running_var, momentum, d_gamma, d_beta, eps, d_scale, d_shift);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

// Backward of training-mode BatchNorm (optionally with the ReLU that follows it: pass its output d_y, else NULL):
// d_dgamma, d_dbeta, d_dx, and optionally d_dres = the ReLU-masked incoming gradient (gradient of a residual
// that was added between the normalisation and the ReLU).
static int bn_backward_impl(const float* d_x, const float* d_dy, const float* d_y, long long n, int c, int ld,
                            const float* d_mean, const float* d_var, float eps, const float* d_gamma, float* d_dgamma,
                            float* d_dbeta, float* d_dx, float* d_dres, void* d_ws, size_t ws_bytes, float* d_dx_hl,
                            unsigned* d_slot, int32_t* range_flag, const unsigned* d_relu_bits, void* stream) {
    CV_REQUIRE(d_x && d_dy && d_mean && d_var && d_gamma && d_dgamma && d_dbeta && d_dx && d_ws, CV_EINVAL, "null pointer argument");
    CV_REQUIRE(n > 0 && c > 0 && ld >= c, CV_EINVAL, "bad bn sizes");
    CV_REQUIRE(ws_bytes >= cv_sp_bn_workspace_bytes(c), CV_ENOMEM, "workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(d_ws);
    const int chunks = bn_chunks(n);
    dim3 grid((unsigned)((c + 31) / 32), (unsigned)chunks);
    const bool v4 = c % 4 == 0 && c <= 1024 && ld % 4 == 0 && aligned16(d_x) && aligned16(d_dy) && aligned16(d_y) &&
                    aligned16(d_dx) && aligned16(d_dres) && aligned16(d_mean) && aligned16(d_var);
    CV_REQUIRE(!d_relu_bits || (v4 && c % 32 == 0), CV_EINVAL, "ReLU bits: c %% 32 == 0 and 16-byte aligned operands");
    if (v4)
        bn_col_reduce4<1><<<chunks, 256, 0, st>>>(d_x, d_dy, d_y, n, c, ld, d_mean, d_var, eps, partial, d_relu_bits);
    else
        bn_col_reduce<1><<<grid, 256, 0, st>>>(d_x, d_dy, d_y, n, c, ld, d_mean, d_var, eps, partial);
    CV_LAUNCH_CHECK();
    bn_col_finish<1><<<(c + 15) / 16, 256, 0, st>>>(partial, chunks, n, c, d_dbeta, d_dgamma, nullptr, nullptr, 0.f,
                                                     nullptr, nullptr, eps, nullptr, nullptr);
    CV_LAUNCH_CHECK();
    CV_REQUIRE(!d_dx_hl || (v4 && d_slot && c % 32 == 0 && ld % 32 == 0 && (reinterpret_cast<uintptr_t>(d_dx_hl) & 127) == 0), CV_EINVAL,
               "hl-format gradient: channels and leading dimension %% 32 == 0, 128-byte aligned rows, a scale slot");
    if (v4)
        bn_backward_apply4<<<(unsigned)std::min<long long>((n * (c / 4) + 255) / 256, d_dx_hl ? BN_SLOT_BLOCKS : 16384), 256, 0, st>>>(
            d_x, d_dy, d_y, n, c, ld, d_mean, d_var, eps, d_gamma, d_dbeta, d_dgamma, d_dx, d_dres, d_dx_hl, d_slot, range_flag, d_relu_bits);
    else
        bn_backward_apply<<<(unsigned)std::min<long long>((n * c + 255) / 256, 8192), 256, 0, st>>>(
            d_x, d_dy, d_y, n, c, ld, d_mean, d_var, eps, d_gamma, d_dbeta, d_dgamma, d_dx, d_dres);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_sp_bn_backward_f32(const float* d_x, const float* d_dy, const float* d_y, long long n, int c, int ld,
                          const float* d_mean, const float* d_var, float eps, const float* d_gamma, float* d_dgamma,
                          float* d_dbeta, float* d_dx, float* d_dres, void* d_ws, size_t ws_bytes, void* stream) {
    return bn_backward_impl(d_x, d_dy, d_y, n, c, ld, d_mean, d_var, eps, d_gamma, d_dgamma, d_dbeta, d_dx, d_dres, d_ws, ws_bytes,
                            nullptr, nullptr, nullptr, nullptr, stream);
}

int cv_sp_bn_backward_hl_f32(const float* d_x, const float* d_dy, const float* d_y, long long n, int c, int ld,
                             const float* d_mean, const float* d_var, float eps, const float* d_gamma, float* d_dgamma,
                             float* d_dbeta, float* d_dx, float* d_dres, void* d_ws, size_t ws_bytes, float* d_dx_hl,
                             uint32_t* d_slot, int32_t* range_flag, const uint32_t* d_relu_bits, void* stream) {
    CV_REQUIRE((d_dx_hl != nullptr) == (d_slot != nullptr), CV_EINVAL, "the hl twin of dx and its scale slot come together");
    return bn_backward_impl(d_x, d_dy, d_y, n, c, ld, d_mean, d_var, eps, d_gamma, d_dgamma, d_dbeta, d_dx, d_dres, d_ws, ws_bytes,
                            d_dx_hl, d_slot, range_flag, d_relu_bits, stream);
}

}  // extern "C"
