// Sparse convolution for gfx950 as an output-stationary implicit GEMM on the matrix cores: the front door.
// The dispatcher (cv_sp_conv_f32, cv_sp_conv_models_f32: every choice of which kernel runs and how it is sized, every check),
// its options, the stem kernel (conv_stem_mfma) and the finish kernels (conv_finish*).  The product kernels are one file per
// family - conv_rows.hip, conv_rows_wp.hip, conv_hl.hip, conv_hd.hip - behind the launchers of sparse_conv_common.h;
// weight packers and mask orders are conv_prep.hip, row kernels and heads row_ops.hip, the weight gradient sparse_train.hip.
//
// Supplies the arithmetic the reference gets from MinkowskiEngine [ME-ext]:
//   MinkowskiConvolution / ConvolutionTranspose  (utils/minkunet.py:53-119, utils/resnet.py:128-133)
//   MinkowskiBatchNorm (eval: per-channel affine), MinkowskiReLU, the residual add of
//   BasicBlock (utils/resnet.py:118-154 via ME BasicBlock) and `final`'s bias
//   out[u] = sum_j W_j^T x[nbr[u][j]]  over valid neighbours,  W = `kernel` [K][Cin][Cout]
//
// Precision: the reference network is fp32 (train_joint.py:219-223, no autocast) and the
// parity bar is 1e-4 on its outputs, so the GEMM runs on v_mfma_f32_32x32x2_f32: exact fp32
// products and fp32 accumulation at the fp32 matrix rate (157 TF/s peak; gfx950 has no
// xf32/tf32 path).  That is conv_rows; the piece-product kernels (conv_rows_wp, conv_hl, conv_hd) form the same products
// from bf16 / fp16 pieces on the 16-bit matrix pipes.
//
// Small coordinate sets (coarse levels: hundreds of rows x 256 channels) split the kernel offsets over
// blockIdx.z into a workspace that conv_finish reduces (+ epilogue).
// Fine-grained sparsity: only ~23-50 % of (row, offset) pairs exist, but a 32-row MFMA block is live as
// soon as ONE of its rows has the neighbour.  The caller may therefore pass a processing order
// (row_perm) that groups rows with equal neighbour bit masks and run the offsets in two halves, each
// with the order sorted by that half's mask: 32-row blocks then need 29-55 % of the offsets instead of
// 90 %, and dead waves / tiles skip their MFMAs / staging.
#include "cv_common.h"

#include <atomic>
#include <cstring>
#include <type_traits>
#include <utility>

#include "sparse_conv_common.h"

using namespace cvsc;

namespace {

// ------------------------------------------------------------------ stem on the matrix cores (fp16 pairs)
// conv0p1s1 (utils/minkunet.py:53: 5x5x5, 3 or 6 -> 32 channels): 13 % of the 125 (row, offset) pairs exist.  Rounds 1-5 also
// kept a lane-per-row stem on the vector ALUs (one lane = one output row and all 32 outputs in registers, weights through the
// scalar cache; 93-107 us at 80k rows, removed in round 6: the training forward takes this kernel too, other fp32 callers the
// generic conv_rows): it executed 32*CIN FMAs for every offset ANY of a wave's 64 rows had (~90 % of the 125).  As a GEMM over the gathered operand
// [rows][CIN * 128] (offsets padded to 128, dead entries zero) it is 1.97 GFLOP dense - nothing for the matrix cores -
// and what remains is what the stem really is: 125 map entries and ~16 gathers of CIN floats per row.
// A wave owns 32 rows; per group of 16 offsets a lane (row = lane % 32, half = lane / 32) reads its row's 8 map
// entries, gathers the CIN floats of the existing ones, splits them into fp16 pairs (split2h) and feeds CIN x 3
// v_mfma_f32_32x32x16_f16 (k = the 16 offsets of the group, one MFMA triple per input channel).  The weights
// (cv_sp_pack_weights_stem_h2_f32: BatchNorm scale and a power of two folded in, fp16 pairs in B-operand order,
// 16 KB per input channel) sit in LDS for the whole workgroup.  Same products as the fp32 chain to 2^-22, fp32 accumulation.
template <int CIN, class... MA>       // (MA: empty or one ModelArgs - blockIdx.y = model; the input rows are shared)
__global__ __launch_bounds__(THREADS, (CIN <= 3 ? 3 : 1)) void conv_stem_mfma(ConvArgs a, MA... ma) {
    model_enter_y(a, ma...);
    constexpr int G = 8;                              // groups of 16 kernel offsets (K <= 128)
    constexpr int W_BYTES = G * CIN * 2 * 1024;       // [group][channel][plane][col][half][8] fp16
    constexpr int EP_BYTES = 4 * 32 * EP_LD * 4;
    constexpr int SM_BYTES = W_BYTES > EP_BYTES ? W_BYTES : EP_BYTES;
    __shared__ __attribute__((aligned(16))) unsigned char w_s[SM_BYTES];    // the weights; then the epilogue tile
    __shared__ int rows_s[TM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const long long r0 = (long long)blockIdx.x * TM;
    for (int f = tid; f < W_BYTES / 16; f += THREADS)
        reinterpret_cast<uint4*>(w_s)[f] = reinterpret_cast<const uint4*>(a.wp6)[f];
    if (tid < TM) rows_s[tid] = r0 + tid < a.n_out ? (int)(r0 + tid) : -1;
    const long long row = r0 + wave * 32 + l31;
    const bool have = row < a.n_out;
    const int K = a.K;
    const int* __restrict__ mrow = a.nbr + (have ? row : 0) * (long long)K;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float in_max = 0.f;
    // every map entry of the lane's row half first (64 independent loads in flight: the map is streamed from HBM / the
    // Infinity Cache once), then the groups with the gathers one group ahead of the MFMAs
    int m[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = g * 16 + half * 8 + i;
            m[g][i] = (have && j < K) ? mrow[j] : -1;
        }
    float x0[8][CIN], x1[8][CIN];
    auto gather = [&](const int* mg, float (*x)[CIN]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (mg[i] >= 0) {
                const float* p = a.in + (long long)mg[i] * a.in_ld;
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci) x[i][ci] = p[ci];
            } else {
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci) x[i][ci] = 0.f;
            }
        }
    };
    gather(m[0], x1);
    __syncthreads();                                  // weights in LDS
#pragma unroll
    for (int g = 0; g < G; ++g) {
        bool any = false;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) x0[i][ci] = x1[i][ci];
            any |= m[g][i] >= 0;
        }
        if (g + 1 < G) gather(m[g + 1], x1);
        if (__any(any)) {
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) {
                unsigned h[4], l[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    in_max = fmaxf(in_max, fmaxf(fabsf(x0[2 * q][ci]), fabsf(x0[2 * q + 1][ci])));
                    split2h(x0[2 * q][ci], x0[2 * q + 1][ci], h[q], l[q]);
                }
                const f16x8 a0 = __builtin_bit_cast(f16x8, make_uint4(h[0], h[1], h[2], h[3]));
                const f16x8 a1 = __builtin_bit_cast(f16x8, make_uint4(l[0], l[1], l[2], l[3]));
                const unsigned char* wb = w_s + ((g * CIN + ci) * 2) * 1024 + (l31 * 2 + half) * 16;
                const f16x8 b0 = *reinterpret_cast<const f16x8*>(wb);
                const f16x8 b1 = *reinterpret_cast<const f16x8*>(wb + 1024);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, acc, 0, 0, 0);
            }
        }
    }
    if (in_max > 65000.f && a.range_flag) *a.range_flag = 1;
    {
        const float sc = a.acc_scale_dev ? a.acc_scale * *a.acc_scale_dev : a.acc_scale;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] *= sc;
    }
    __syncthreads();                                  // the weights are dead: the epilogue tile reuses their LDS
    float (*ep)[EP_LD] = reinterpret_cast<float (*)[EP_LD]>(w_s + wave * 32 * EP_LD * 4);
    epilogue_store_wide(a, acc, rows_s + wave * 32, 0, lane, ep);
}

// sums the per-split partial tiles and applies the epilogue (scale/shift/residual/relu).
// One thread per 4 consecutive columns (float4 loads, cout % 4 == 0) and per quarter of the splits;
// the four quarter-sums meet through LDS, so small outputs with many splits still have enough loads
// in flight (a one-thread-per-element loop over 64 splits ran at 1.7 TB/s).
// (MA, here and in the two kernels below: empty, or one ModelArgs - blockIdx.y = model, the grid-stride loop over x unchanged)
template <class... MA>
__global__ __launch_bounds__(256) void conv_finish(ConvArgs a, MA... ma) {
    model_enter_y(a, ma...);
    __shared__ float4 red[4][64];
    const int q = threadIdx.x >> 6, l = threadIdx.x & 63;
    const long long total4 = a.n_out * (long long)a.cout / 4;
    const long long total = a.n_out * (long long)a.cout;
    for (long long base = blockIdx.x * 64ll; base < total4; base += (long long)gridDim.x * 64) {
        const long long e4 = base + l;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e4 < total4) {
            const float4* p = reinterpret_cast<const float4*>(a.partial) + e4;
#pragma unroll 4
            for (int k = q; k < a.splits; k += 4) {
                const float4 v = partial_load4(p + (long long)k * (total / 4));
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
        }
        red[q][l] = s;
        __syncthreads();
        if (q == 0 && e4 < total4) {
            float v[4] = {red[0][l].x + red[1][l].x + red[2][l].x + red[3][l].x,
                          red[0][l].y + red[1][l].y + red[2][l].y + red[3][l].y,
                          red[0][l].z + red[1][l].z + red[2][l].z + red[3][l].z,
                          red[0][l].w + red[1][l].w + red[2][l].w + red[3][l].w};
            const long long e = e4 * 4;
            const long long row = e / a.cout;
            const int col = (int)(e - row * a.cout);
            if (a.wide) {                        // 16-byte aligned operands: one float4 per operand instead of four words
                epilogue_apply4(a, row, col, make_float4(v[0], v[1], v[2], v[3]));
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) epilogue_apply1(a, row, col + i, v[i]);
            }
        }
        __syncthreads();
    }
}

// up to FINISH_SMALL_MAX partial tiles (the mask groups, the split-K of the middle levels) with 16-byte aligned
// operands: a thread owns a float4 of the output, has all its partial loads in flight at once and runs the epilogue
// itself - no LDS exchange, no barriers, every thread stores (ts1 96 -> 96 conv + finish: 125 -> 104 us).  Summation
// order = conv_finish's: four running sums (from +0) over the partials k % 4, then ((s0 + s1) + s2) + s3 - bit-identical results.
//   - instances per class of the split count (SMAX = 4, 8, 16 slots: three mask groups do not carry sixteen predicated
//     slots - 23 / 40 / 72 VGPRs, it was one instance of 80);
//   - IDX: item, row and column arithmetic in 32 bits where n_out * cout fits (the host decides), else in 64;
//   - no grid cap and no stride loop: the grid covers the items.
// Which partials exist comes as ONE word per row, loaded in front of the partials: w & gm.m[k] != 0 = partial k of the row was
// written.  Without validity data (a.gvalid NULL) the word is all ones and m[k] is all ones for k < splits, 0 behind; with it
// (zskip) the word is the row's validity word and m[k] the bits of mask group k's offsets.  A partial that was not written
// is not loaded (zskip saves the read as well as the write) and adds +0 in its place - the adds of zero stay, they decide the
// sign of a zero sum.
// Measured and dropped (LABNOTES "Zero tiles", profiles/zero_tiles/rates_variants.txt; parent 655-672 scenes/s seven in flight):
// a thread that owns 8 columns (two float4 per partial, 16-byte hl stores) 651-661, several items per thread with every load of
// all of them issued first 633-657 (8 columns) / 667-679 (4 columns x 2) against 676-682 for this form - a lane that owns 32 bytes
// of a row halves what one load instruction of the wave covers contiguously, and fatter threads only cost registers (118 / 220
// VGPRs) on a chip that other scenes' waves already fill.
constexpr int FINISH_SMALL_MAX = 16;
template <int SMAX> struct FinishMasks { unsigned m[SMAX]; };

template <int SMAX, class IDX, class... MA>
__global__ __launch_bounds__(256) void conv_finish_small(ConvArgs a, FinishMasks<SMAX> gm, MA... ma) {
    model_enter_y(a, ma...);
    const IDX cq = (IDX)(a.cout >> 2);
    const IDX total4 = (IDX)a.n_out * cq;
    const IDX e4 = (IDX)blockIdx.x * (IDX)256 + (IDX)threadIdx.x;
    if (e4 >= total4) return;
    const IDX row = e4 / cq;
    const int col = (int)(e4 - row * cq) * 4;
    const unsigned w = a.gvalid ? (unsigned)a.gvalid[row] : ~0u;
    const float4* p = reinterpret_cast<const float4*>(a.partial) + e4;
    float4 pv[SMAX];
#pragma unroll
    for (int k = 0; k < SMAX; ++k)
        pv[k] = (w & gm.m[k]) ? partial_load4(p + (long long)k * (long long)total4) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 sq[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) sq[q] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < SMAX; ++k)
        if (k < a.splits) { sq[k & 3].x += pv[k].x; sq[k & 3].y += pv[k].y; sq[k & 3].z += pv[k].z; sq[k & 3].w += pv[k].w; }
    const float4 x = make_float4(sq[0].x + sq[1].x + sq[2].x + sq[3].x, sq[0].y + sq[1].y + sq[2].y + sq[3].y,
                                 sq[0].z + sq[1].z + sq[2].z + sq[3].z, sq[0].w + sq[1].w + sq[2].w + sq[3].w);
    epilogue_apply4(a, (long long)row, col, x);
}

// scalar variant for cout % 4 != 0
template <class... MA>
__global__ __launch_bounds__(256) void conv_finish_scalar(ConvArgs a, MA... ma) {
    model_enter_y(a, ma...);
    const long long total = a.n_out * (long long)a.cout;
    for (long long t = blockIdx.x * 256ll + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long row = t / a.cout;
        const int col = (int)(t - row * a.cout);
        float v = 0.f;
        for (int sidx = 0; sidx < a.splits; ++sidx) v += a.partial[sidx * total + t];
        epilogue_apply1(a, row, col, v);
    }
}

// conv_finish_small's instance for (split-count class, index width), its masks and its grid
template <int SMAX, class IDX>
void launch_finish_small(const ConvArgs& a, hipStream_t st, const ModelArgs* ma, int models) {
    FinishMasks<SMAX> gm;
    for (int k = 0; k < SMAX; ++k) {
        gm.m[k] = k < a.splits ? ~0u : 0u;
        if (a.gvalid && k < a.splits) {      // (K <= 32, the dispatcher's condition) group k's offsets, as the kernels and the orders split them
            const int jb = a.K * k / a.splits, je = a.K * (k + 1) / a.splits;
            gm.m[k] = (unsigned)(((1ull << je) - 1) & ~((1ull << jb) - 1));
        }
    }
    const long long items = a.n_out * (long long)a.cout / 4;
    const dim3 grid((unsigned)((items + 255) / 256), (unsigned)models);
    with_models(ma, [&](auto... m) { conv_finish_small<SMAX, IDX, decltype(m)...><<<grid, 256, 0, st>>>(a, gm, m...); });
}

std::atomic<int> g_ablation{0};
// reduce the partial tiles + epilogue (ma: over `models` models, blockIdx.y; the same kernel choice and x grid per model)
int launch_finish(const ConvArgs& a, hipStream_t st, const ModelArgs* ma, int models) {
    if (g_ablation.load(std::memory_order_relaxed) & 1) return CV_OK;      // cv_sp_set_ablation: timing only
    const long long total = a.n_out * (long long)a.cout;
    const auto grid = [&](long long items, int per_block, long long cap) {      // items: float4s or words of the output
        return dim3((unsigned)std::min<long long>((items + per_block - 1) / per_block, cap), (unsigned)models);
    };
    if (a.wide && a.splits <= FINISH_SMALL_MAX) {
        const auto with_idx = [&](auto smax) {
            if (total < (1ll << 31)) launch_finish_small<smax.value, unsigned>(a, st, ma, models);
            else launch_finish_small<smax.value, long long>(a, st, ma, models);
        };
        if (a.splits <= 4) with_idx(std::integral_constant<int, 4>{});
        else if (a.splits <= 8) with_idx(std::integral_constant<int, 8>{});
        else with_idx(std::integral_constant<int, FINISH_SMALL_MAX>{});
    } else if (a.cout % 4 == 0)
        with_models(ma, [&](auto... m) { conv_finish<decltype(m)...><<<grid(total / 4, 64, 8192), 256, 0, st>>>(a, m...); });
    else
        with_models(ma, [&](auto... m) { conv_finish_scalar<decltype(m)...><<<grid(total, 256, 4096), 256, 0, st>>>(a, m...); });
    CV_LAUNCH_CHECK();
    return CV_OK;
}

// run-time options (cv_sp_set_option): conv_hd switch (bit NB - 1) and its row threshold; defaults from the environment
// defaults (profiles/r4/hd2_grid.txt, hd_shapes.txt): the 96-column fine-level launches (>= 16384 rows) on conv_hd, 8 waves x 2 ring
// stages: 558 -> 573 scenes/s with eight scenes in flight (528 -> 575 under the one-call scene path); 32- and 64-column
// launches and the coarse levels stay on conv_hl (conv_hd measured slower there)
// zskip (ON): 12-18 % of the (mask group, 128-row tile) pairs of a mask-sorted level hold no row with a neighbour in the group
// (profiles/zero_tiles/dead_pairs.txt); those tiles write no partial tile and the finish launch loads none for such
// (group, row) pairs.  Round 5 read three validity bytes per finish thread, each load in front of its partial's: 570 against
// 577 scenes/s, off.  Since the rebuilt conv_finish_small the validity is ONE word per row (cv_conv_desc.valid_words: the scene
// plan's word behind every 3x3x3 map), loaded in front of all partials: 84 MB less written and 39 MB less fetched per scene,
// 679-682 against 665-675 scenes/s with the switch off and 664-666 for the parent, five alternated rounds (LABNOTES "Zero
// tiles", profiles/zero_tiles/).  The words are the caller's: the library cannot check them against nbr, wrong words give wrong
// sums.  The C ABI executor entry points (cv_net_run_f32, cv_net_run_models_f32) hand none over - the switch acts in the scene
// calls and on cv_sp_conv_f32 descriptors that carry the words.
std::atomic<long long> g_opt_zskip{getenv("CV_ZSKIP") ? atoll(getenv("CV_ZSKIP")) : 1};
std::atomic<long long> g_zskip_launches{0};      // "zskip_launches": convolutions dispatched with validity words so far (tests: did the switch engage?)
std::atomic<long long> g_opt_hd_mask{getenv("CV_HD") ? atoll(getenv("CV_HD")) : 4};
std::atomic<long long> g_opt_hd_min_rows{getenv("CV_HD_MIN_ROWS") ? atoll(getenv("CV_HD_MIN_ROWS")) : 16384};
std::atomic<long long> g_opt_hd_shape{getenv("CV_HD_SHAPE") ? atoll(getenv("CV_HD_SHAPE")) : 2};      // 0: 8 waves x 3 stages, 1: 4 x 2, 2: 8 x 2

// ma / models: the launch covers `models` models (cv_sp_conv_models_f32): grid.y = models x column blocks, the kernels' ModelArgs instantiations
// NB: 32-column blocks per workgroup (nb_for)
int launch_rows(ConvArgs a, const int NB, bool vec, hipStream_t st, ModelArgs* ma, int models) {
    dim3 grid((unsigned)((a.n_out + TM - 1) / TM), (unsigned)((a.cout + NB * 32 - 1) / (NB * 32)),
              (unsigned)a.splits);
    int per_wg = 0;                                  // most offsets one workgroup walks (the kernel's own formulas)
    if (vec) {
        const int nj_wp = a.j_end - a.j_begin, nch_wp = a.cin / KC;
        for (int z = 0; z < a.splits; ++z) {
            long long lo, hi;
            if (a.perm_per_split) {
                lo = (long long)nj_wp * z / a.splits * nch_wp;
                hi = (long long)nj_wp * (z + 1) / a.splits * nch_wp;
            } else {
                lo = (long long)nj_wp * nch_wp * z / a.splits;
                hi = (long long)nj_wp * nch_wp * (z + 1) / a.splits;
            }
            if (hi > lo) per_wg = std::max(per_wg, (int)((hi - 1) / nch_wp - lo / nch_wp + 1));
        }
    }
    if (ma) {
        CV_REQUIRE(a.in_hl && !a.tickets, CV_EINVAL,
                   "the model axis runs fp16-pair programs on hl buffers only (no fp32 / bf16 convolution, no split_tickets)");
        ma->ncb = (int)grid.y;
        grid.y *= (unsigned)models;
    }
    if (a.in_hl) {
        CV_REQUIRE(per_wg * (a.cin / KC) + (a.in2 ? a.cin2 / KC : 0) <= HL_MAX_UNITS, CV_EINVAL,
                   "hl-format convolution: more than %d units per workgroup (Cin too wide)", HL_MAX_UNITS);
        CV_REQUIRE(vec && a.wp6 && a.pieces == 2 && a.wide && per_wg <= WP_NPRE && NB <= 4, CV_EINVAL,
                   "hl-format input needs the fp16-pair weights, Cin %% 32 == 0, 16-byte aligned operands and at most %d "
                   "kernel offsets per workgroup", WP_NPRE);
        // (measured and dropped, profiles/r2/hl_burst.txt: a variant for workgroups of <= 8 units with every weight tile
        // requested at once through global_load_lds and two dependent round trips instead of 3 + units - no faster)
        // (NS = 8 / 6 / 4 slots for NB = 1 / 2 / 3 measured: every layer 25-45 % slower - two workgroups per CU
        // instead of three or four cost more than the deeper prefetch gains, profiles/r2/hl_slots.txt)
        // conv_hd (round 4): LDS-DMA operand rings, 256-row workgroups; CV_HD bit NB - 1 switches the NB x 32-column kernel on
        // for launches of at least CV_HD_MIN_ROWS output rows
        const int hd_mask = (int)g_opt_hd_mask.load(std::memory_order_relaxed);
        const long long hd_min_rows = g_opt_hd_min_rows.load(std::memory_order_relaxed);
        const int hd_shape = (int)g_opt_hd_shape.load(std::memory_order_relaxed);
        const bool hd = NB <= 3 && ((hd_mask >> (NB - 1)) & 1) && a.n_out >= hd_min_rows;
        // split-K reduced by the last-arriving workgroup (conv_hl) for callers that pass cv_conv_desc.split_tickets: bit-identical to
        // the finish launch (tests); the network executor does not hand tickets over (net_exec.cpp: measured slower)
        if (hd || !(a.splits > 1 && !a.perm_per_split && (long long)grid.x * grid.y <= CV_SPLIT_TICKETS)) a.tickets = nullptr;
        if (hd) {
            const int nw = hd_shape == 1 ? 4 : 8;      // waves = 32-row blocks of a workgroup
            launch_conv_hd(a, NB, hd_shape, ma, dim3((unsigned)((a.n_out + nw * 32 - 1) / (nw * 32)), grid.y, grid.z), st);
        } else {
            launch_conv_hl(a, NB, ma, grid, st);
        }
    } else if (vec && a.wp6 && per_wg <= WP_NPRE) {
        launch_conv_rows_wp(a, NB, a.pieces, false, grid, st);
    } else if (vec && a.wp6 && per_wg <= WP_NPRE_BIG) {
        // more offsets per workgroup than the default instance prefetches (flavour 1 with a whole 3x3x3 kernel, mask groups of
        // > 10 offsets): the instance that keeps 28 map rows per tile (more LDS, fewer workgroups per CU)
        launch_conv_rows_wp(a, NB, a.pieces, true, grid, st);
    } else {
        CV_REQUIRE(a.pieces != 1 || !(vec && a.wp6), CV_EINVAL, "the bf16 compute mode takes at most %d kernel offsets per workgroup", WP_NPRE_BIG);
        // conv_rows knows one source: a launch that reached it with in2 set would return CV_OK without in2 @ W2
        CV_REQUIRE(!a.in2, CV_EINVAL,
                   "a second source takes at most %d kernel offsets per workgroup (%d here: flavour 0 with a workspace splits the "
                   "launch, or pass fewer offsets per call)", WP_NPRE_BIG, per_wg);
        launch_conv_rows(a, NB, vec, grid, st);
    }
    CV_LAUNCH_CHECK();
    return a.splits > 1 && !a.tickets ? launch_finish(a, st, ma, models) : CV_OK;
}

// 32-column blocks per workgroup.  Wider than 96 columns is split over blockIdx.y in 64-column workgroups: measured 118 -> 97 us (2349 rows, 256 -> 256), 143 -> 117 us (9929 rows, 128 -> 128),
// 40 -> 33 us (494 rows) against 128-column workgroups - more, lighter workgroups hide the gather latency better
// than the saved operand re-reads are worth; 96 columns stay one workgroup (64 + 32 is uneven: 144 -> 180 us).
int nb_for(int cout) {
    static const int nb_max = getenv("CV_NB_MAX") ? atoi(getenv("CV_NB_MAX")) : 0;
    if (nb_max > 0) return std::min(nb_max, nb_full(cout));
    if (cout <= 32) return 1;
    if (cout <= 64) return 2;
    if (cout <= 96) return 3;
    static const int nb_wide = getenv("CV_NB_WIDE") ? atoi(getenv("CV_NB_WIDE")) : 2;      // 128 / 256 columns: 64-column workgroups
    // (until round 5 the levels below 1024 rows took 32-column workgroups - measured with the fp32-row kernels of round 1; on the hl
    // kernels 64 columns are better alone and with scenes in flight: net 2.32 -> 2.29-2.30 ms, 592 -> 599-600 scenes/s,
    // profiles/r5/nb_coarse.txt; 96 / 128 columns: 591 / 583)
    return std::max(1, std::min(nb_wide, 2));
}

// workgroups a split launch aims at: CV_SPLIT_TARGET or 768 until cv_sp_set_split_target changes it
std::atomic<long long> g_split_target{-1};
thread_local long long t_split_target = 0;       // cv_sp_set_split_target_thread: this thread's launches (0 = the process-wide value)
long long process_split_target() {
    long long v = g_split_target.load(std::memory_order_relaxed);
    if (v <= 0) {
        v = getenv("CV_SPLIT_TARGET") ? std::max(1ll, atoll(getenv("CV_SPLIT_TARGET"))) : 768;
        g_split_target.store(v, std::memory_order_relaxed);
    }
    return v;
}
long long split_target() { return t_split_target > 0 ? t_split_target : process_split_target(); }

// Enough workgroups to fill 256 CUs a few times with short dependent chains: split the (offset,
// chunk) units over blockIdx.z; the partial tiles cost 8 bytes of traffic per output element per split.
int pick_splits(long long n_out, int cout, int K, int cin, bool vec) {
    const int nb = nb_for(cout);
    const long long tiles = ((n_out + TM - 1) / TM) * ((cout + nb * 32 - 1) / (nb * 32));
    const long long units = vec ? (long long)K * (cin / KC) : ((long long)K * cin + KC - 1) / KC;
    if (tiles >= 384 || units <= 1) return 1;
    // workgroups a split launch aims at.  768 since round 5 (the one-scene-at-a-time optimum on the hl kernels: 384 / 512 / 768 /
    // 1024 = 339 / 341-344 / 347.0 / 347.2 scenes/s one in flight, profiles/r5/one_in_flight_defaults.txt; hosts with scenes in flight
    // set their own value).  512 from round 2 on: 384 / 512 / 768 / 1024 = 513 / 508 / 496 / 491 scenes/s six in
    // flight, net 2.58 / 2.51 / 2.47 / 2.47 ms one in flight - the partial tiles of the coarse levels are 0.8 GB of the
    // 1.7 GB a forward writes, and with several scenes in flight the other scenes fill the chip, not the splits
    // (cv_sp_set_split_target: with EIGHT scenes in flight 256 gives 562-566 scenes/s against 550 for 512 and 549-555
    // for 128, profiles/r3/split_target_8streams.txt - the host picks the value by how many scenes it keeps in flight)
    const long long target = split_target();
    long long s = (target + tiles - 1) / tiles;
    // (measured without gain: sizing by the chip's resident workgroup slots, floor(256 x waves-per-SIMD / tiles), so that
    // no second round of workgroups starts: 257 vs 265 scenes/s one scene in flight, 401-409 vs 410-412 with six)
    s = std::min(s, units);
    static const long long traffic_mb = getenv("CV_SPLIT_TRAFFIC_MB") ? atoll(getenv("CV_SPLIT_TRAFFIC_MB")) : 24;
    const long long by_traffic = (traffic_mb << 20) / std::max<long long>(1, n_out * cout * 4);   // <= 24 MB of partials
    s = std::min(s, std::max<long long>(by_traffic, 2));
    s = std::min<long long>(s, 64);
    return (int)std::max<long long>(s, 1);
}

}  // namespace

static std::atomic<long long>* option_named(const char* name) {
    return !strcmp(name, "hd_mask") ? &g_opt_hd_mask : !strcmp(name, "hd_min_rows") ? &g_opt_hd_min_rows :
           !strcmp(name, "hd_shape") ? &g_opt_hd_shape : !strcmp(name, "zskip") ? &g_opt_zskip :
           !strcmp(name, "zskip_launches") ? &g_zskip_launches : nullptr;
}

int cv_sp_set_option(const char* name, long long value, long long* previous) {
    CV_REQUIRE(name, CV_EINVAL, "null option name");
    std::atomic<long long>* o = option_named(name);
    CV_REQUIRE(o, CV_EINVAL, "unknown option '%s' (hd_mask, hd_min_rows, hd_shape, zskip, zskip_launches)", name);
    const long long before = o->exchange(value, std::memory_order_relaxed);
    if (previous) *previous = before;
    return CV_OK;
}

int cv_sp_get_option(const char* name, long long* value) {
    CV_REQUIRE(name && value, CV_EINVAL, "null option name / value");
    const std::atomic<long long>* o = option_named(name);
    CV_REQUIRE(o, CV_EINVAL, "unknown option '%s'", name);
    *value = o->load(std::memory_order_relaxed);
    return CV_OK;
}

int cv_sp_set_ablation(int bits) { return g_ablation.exchange(bits, std::memory_order_relaxed); }

int cv_sp_set_split_target_thread(int workgroups) {
    const int before = (int)t_split_target;
    t_split_target = workgroups > 0 ? workgroups : 0;
    return before;
}

int cv_sp_set_split_target(int workgroups) {
    const int before = (int)process_split_target();          // (the process-wide value, whatever the calling thread's own is)
    g_split_target.store(workgroups > 0 ? workgroups : -1, std::memory_order_relaxed);
    return before;
}

static int conv_dispatch(const cv_conv_desc* d, const CvConvModels* mm, void* stream);

extern "C" {

size_t cv_sp_conv_workspace_bytes(long long n_out, int cout, int K) {
    if (n_out <= 0 || cout <= 0 || K <= 0) return 0;
    const size_t one = sizeof(float) * (size_t)n_out * (size_t)cout;
    return 256 + std::min<size_t>(64 * one, std::max<size_t>((size_t)48 << 20, 3 * one));   // see pick_splits (and the
                                                                                            // 3-way split of conv_hl)
}

int cv_sp_conv_f32(const cv_conv_desc* d, void* stream) { return conv_dispatch(d, nullptr, stream); }

}  // extern "C"

int cv_sp_conv_models_f32(const cv_conv_desc* d, const CvConvModels* mm, void* stream) {
    CV_REQUIRE(d && mm && mm->d_params && mm->models >= 1 && mm->models <= CV_MAX_CATEGORIES, CV_EINVAL, "bad model-axis arguments");
    CV_REQUIRE(!d->split_tickets, CV_EINVAL, "the model axis does not take split_tickets");
    CV_REQUIRE(d->weight_pieces == 2 && !d->acc_in && !d->acc_scale_dev, CV_EINVAL,
               "the model axis runs fp16-pair programs only (weight_pieces == 2; no bf16 triples, no fp32 convolution)");
    CV_REQUIRE(((mm->in_stride | mm->in2_stride | mm->res_stride | mm->out_stride | mm->ws_stride) & 127) == 0, CV_EINVAL,
               "model strides must keep rows 128-byte aligned");
    return conv_dispatch(d, mm, stream);
}

// mm: the launches cover mm->models models (cv_sp_conv_models_f32); every choice below is made from ONE model's sizes
static int conv_dispatch(const cv_conv_desc* d, const CvConvModels* mm, void* stream) {
    CV_REQUIRE(d, CV_EINVAL, "null descriptor");
    CV_REQUIRE(d->in && d->weight && d->out, CV_EINVAL, "null pointer argument");
    CV_REQUIRE(d->n_in > 0 && d->n_out > 0 && d->cin > 0 && d->cout > 0 && d->K > 0, CV_EINVAL, "bad conv sizes");
    CV_REQUIRE(d->nbr || (d->K == 1 && d->n_in == d->n_out), CV_EINVAL, "a kernel map is required unless K == 1");
    CV_REQUIRE(d->in_ld >= d->cin && d->out_ld >= d->cout && (!d->residual || d->res_ld >= d->cout) &&
                   (!d->acc_in || d->acc_ld >= d->cout), CV_EINVAL, "bad leading dimension");
    CV_REQUIRE(d->out != d->in, CV_EINVAL, "conv cannot run in place");
    const int jb = d->j_begin, je = d->j_end > 0 ? d->j_end : d->K;
    CV_REQUIRE(jb >= 0 && jb < je && je <= d->K, CV_EINVAL, "bad kernel offset range");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ConvArgs a = {};           // what is not named here is zero / NULL until the route below sets it
    a.in = d->in, a.n_in = d->n_in, a.in_ld = d->in_ld, a.cin = d->cin;
    a.w = d->weight, a.K = d->K, a.cout = d->cout;
    a.nbr = d->nbr, a.n_out = d->n_out;
    a.scale = d->scale, a.shift = d->shift;
    a.res = d->residual, a.res_ld = d->res_ld;
    a.relu = d->relu;
    a.out = d->out, a.out_ld = d->out_ld;
    a.splits = 1;
    a.row_perm = d->row_perm;
    a.j_begin = jb, a.j_end = je;
    a.acc_in = d->acc_in, a.acc_ld = d->acc_ld;
    a.wp6 = static_cast<const unsigned short*>(d->weight_x6);
    a.in2 = d->in2, a.in2_ld = d->in2_ld, a.cin2 = d->cin2;
    a.wp6_2 = static_cast<const unsigned short*>(d->weight2_x6);
    a.pieces = d->weight_pieces == 2 ? 2 : d->weight_pieces == 1 ? 1 : 3;
    a.acc_scale = d->acc_scale != 0.f ? d->acc_scale : 1.f;
    a.range_flag = d->range_flag;
    a.in_hl = d->in_hl, a.out_hl = d->out_hl, a.res_hl = d->res_hl;
    a.tickets = d->in_hl ? d->split_tickets : nullptr;       // the in-launch split-K reduction exists in conv_hl only
    if (d->in_hl || d->out_hl || d->res_hl) {
        CV_REQUIRE(!d->in_hl || (d->weight_pieces == 2 && d->cin % 32 == 0 && d->in_ld % 32 == 0 &&
                                 (reinterpret_cast<uintptr_t>(d->in) & 127) == 0 &&
                                 (!d->in2 || (d->cin2 % 32 == 0 && d->in2_ld % 32 == 0 &&
                                              (reinterpret_cast<uintptr_t>(d->in2) & 127) == 0))),
                   CV_EINVAL, "hl-format input: fp16-pair weights, channels and leading dimensions %% 32 == 0, 128-byte aligned rows");
        CV_REQUIRE(!d->out_hl || (d->cout % 32 == 0 && d->out_ld % 32 == 0 && (reinterpret_cast<uintptr_t>(d->out) & 127) == 0),
                   CV_EINVAL, "hl-format output: Cout and leading dimension %% 32 == 0, 128-byte aligned rows");
        CV_REQUIRE(!d->res_hl || !d->residual || (d->res_ld % 32 == 0 && (reinterpret_cast<uintptr_t>(d->residual) & 127) == 0),
                   CV_EINVAL, "hl-format residual: leading dimension %% 32 == 0, 128-byte aligned rows");
        CV_REQUIRE(d->flavour == 0, CV_EINVAL, "the hl format runs with flavour 0 only");
        // conv_hl forms its gather addresses in 32 bits (row * row bytes + chunk offset)
        CV_REQUIRE(!d->in_hl || ((unsigned long long)d->n_in * (unsigned long long)d->in_ld * 4ull + (unsigned long long)d->cin * 4ull < (1ull << 32) &&
                                 (!d->in2 || (unsigned long long)d->n_out * (unsigned long long)d->in2_ld * 4ull + (unsigned long long)d->cin2 * 4ull < (1ull << 32))),
                   CV_EINVAL, "hl-format input larger than 4 GiB (rows x leading dimension x 4): split the batch");
    }
    CV_REQUIRE(d->weight_pieces >= 0 && d->weight_pieces <= 3, CV_EINVAL,
               "weight_pieces is 0/3 (bf16 triples), 2 (fp16 pairs) or 1 (single bf16 product)");
    CV_REQUIRE(d->weight_pieces != 1 || (d->weight_x6 && d->cin % KC == 0), CV_EINVAL,
               "weight_pieces = 1 needs weight_x6 from cv_sp_pack_weights_bf16_f32 and Cin %% 32 == 0");
    const bool stem_h2 = d->weight_pieces == 2 && d->weight_x6 && d->cout == 32 && (d->cin == 3 || d->cin == 6) && d->K <= 128;
    CV_REQUIRE(d->weight_pieces != 2 || stem_h2 || (d->weight_x6 && d->cin % KC == 0), CV_EINVAL,
               "weight_pieces = 2 needs weight_x6 from cv_sp_pack_weights_h2_f32 and Cin %% 32 == 0 (or the stem shape with "
               "cv_sp_pack_weights_stem_h2_f32)");

    ModelArgs ma = {};
    if (mm) {
        ma.params = mm->d_params;
        ma.in_stride = mm->in_stride, ma.in2_stride = mm->in2_stride, ma.res_stride = mm->res_stride, ma.out_stride = mm->out_stride;
        ma.partial_stride = mm->ws_stride;
        ma.out_ext = mm->out_ext;
        for (int m = 0; m < mm->models; ++m) ma.ext_out[m] = mm->ext_out[m];
    }
    ModelArgs* const pma = mm ? &ma : nullptr;
    const int models = mm ? mm->models : 1;
    CV_REQUIRE(!d->plan_ent && !d->plan_cnt && !d->weight_packed && (d->flavour == 0 || d->flavour == 1), CV_EINVAL,
               "flavours 3 / 4 (the experimental wave / tile kernels of rounds 1-3) are gone: flavour is 0 or 1, plan_ent / plan_cnt / "
               "weight_packed must be NULL");
    a.wide = d->cout % 4 == 0 && d->out_ld % 4 == 0 && (!d->residual || d->res_ld % 4 == 0) &&
             (!d->acc_in || d->acc_ld % 4 == 0) &&
             ((reinterpret_cast<uintptr_t>(d->out) | reinterpret_cast<uintptr_t>(d->residual) |
               reinterpret_cast<uintptr_t>(d->acc_in) | reinterpret_cast<uintptr_t>(d->scale) |
               reinterpret_cast<uintptr_t>(d->shift) | reinterpret_cast<uintptr_t>(d->ws)) & 15) == 0;
    // the word-by-word epilogue (epilogue_apply1: epilogue_store, conv_finish's scalar branch, conv_finish_scalar) knows only fp32 operands:
    // an hl output or residual needs the float4 epilogues (as an hl input already does, launch_rows)
    CV_REQUIRE(a.wide || (!d->out_hl && !d->res_hl), CV_EINVAL,
               "hl-format output / residual: Cout, leading dimensions %% 4 == 0 and 16-byte aligned out, residual, acc_in, "
               "scale, shift and ws");
    const bool vec = (d->cin % KC == 0) && (d->in_ld % 4 == 0) && (d->cout % 4 == 0) &&
                     ((reinterpret_cast<uintptr_t>(d->in) & 15) == 0) &&
                     ((reinterpret_cast<uintptr_t>(d->weight) & 15) == 0);
    // packed weights are only read by the vector path: without it the launch would fall back to `weight` - which a caller
    // that packed W^T straight from the forward weights (cv_sp_pack_weights_t_f32) holds in the OTHER layout
    CV_REQUIRE(!d->weight_x6 || vec || stem_h2, CV_EINVAL,
               "weight_x6 needs the vector path: Cin %% 32 == 0, Cout %% 4 == 0, in_ld %% 4 == 0, 16-byte aligned in / weight");
    if (d->in2) {
        CV_REQUIRE(vec && d->weight_x6 && d->weight2_x6 && d->cin2 > 0 && d->cin2 % KC == 0 && d->in2_ld >= d->cin2 &&
                       d->in2_ld % 4 == 0 && (reinterpret_cast<uintptr_t>(d->in2) & 15) == 0,
                   CV_EINVAL, "a second source needs the bf16x6 vector path (weight_x6, weight2_x6, Cin2 %% 32 == 0, "
                              "16-byte aligned rows)");
    }
    if (!vec && d->cout == 32 && (d->cin == 3 || d->cin == 6) && d->nbr && !d->row_perm && d->perm_groups <= 1 &&
        d->flavour == 0) {
        if (d->weight_x6 && d->weight_pieces == 2 && d->K <= 128 && a.wide && !d->acc_in && d->j_begin == 0 &&
            (d->j_end == 0 || d->j_end == d->K)) {
            // matrix-core stem (weights from cv_sp_pack_weights_stem_h2_f32, BatchNorm scale folded in)
            const dim3 g((unsigned)((d->n_out + TM - 1) / TM), (unsigned)models);
            if (d->cin == 3) with_models(pma, [&](auto... m) { conv_stem_mfma<3, decltype(m)...><<<g, THREADS, 0, st>>>(a, m...); });
            else with_models(pma, [&](auto... m) { conv_stem_mfma<6, decltype(m)...><<<g, THREADS, 0, st>>>(a, m...); });
            CV_LAUNCH_CHECK();
            return CV_OK;
        }
    }
    CV_REQUIRE(!mm || d->in_hl, CV_EINVAL, "the model axis runs fp16-pair programs on hl buffers only (and their matrix-core stem)");
    a.acc_scale_dev = d->acc_scale_dev;
    if (d->perm_groups > 1) {
        // offsets split into perm_groups contiguous groups, each processed in its own row order, all in
        // one launch (grid.z); partial tiles are reduced by conv_finish
        const size_t need = sizeof(float) * (size_t)d->perm_groups * (size_t)d->n_out * (size_t)d->cout;
        CV_REQUIRE(d->row_perm && vec && d->ws && d->ws_bytes >= need, CV_EINVAL,
                   "perm_groups needs row_perm[groups][n_out], Cin %% 32 == 0 and a workspace of %zu bytes", need);
        a.splits = d->perm_groups;
        a.perm_per_split = 1;
        a.partial = static_cast<float*>(d->ws);
        if (d->perm_has_map && jb == 0 && je == d->K && d->nbr) {
            a.nbr_perm = d->row_perm + (long long)d->perm_groups * d->n_out;
            a.nbr_perm_w = (d->K + d->perm_groups - 1) / d->perm_groups;
            // zskip: tiles whose rows have no neighbour in their group write no partial tile and the finish launch does not read
            // one (validity: the caller's word per row, cv_conv_desc.valid_words).  Not with a second source (its chunks are
            // dealt to the groups: every row gets a sum from them) and only where conv_finish_small finishes.
            if (g_opt_zskip.load(std::memory_order_relaxed) && d->valid_words && d->K <= 32 && !d->in2 && a.wide &&
                d->perm_groups <= FINISH_SMALL_MAX && d->in_hl) {
                a.gvalid = d->valid_words;
                g_zskip_launches.fetch_add(1, std::memory_order_relaxed);
            }
        }
    } else if (d->flavour == 0) {
        int sp = pick_splits(d->n_out, d->cout, je - jb, d->cin, vec);
        if (d->in_hl || (vec && a.wp6)) {
            // conv_hl / conv_rows_wp keep the map entries of at most WP_NPRE offsets per workgroup: launches that would not
            // be split (>= 384 tiles below the mask-sorting threshold, e.g. 13k rows x 256 columns) are split over just
            // enough workgroups
            const int nj = je - jb;
            const int per_wg = sp <= 1 ? nj : (nj + sp - 1) / sp + 1;
            if (per_wg > WP_NPRE) sp = std::max(sp, (nj + WP_NPRE - 2) / (WP_NPRE - 1));
        }
        const size_t need = sizeof(float) * (size_t)sp * (size_t)d->n_out * (size_t)d->cout;
        CV_REQUIRE(!d->in_hl || sp <= 1 || (d->ws && d->ws_bytes >= need), CV_ENOMEM,
                   "hl-format convolution needs a workspace of %zu bytes (cv_sp_conv_workspace_bytes)", need);
        if (sp > 1 && d->ws && d->ws_bytes >= need) {
            a.splits = sp;
            a.partial = static_cast<float*>(d->ws);
        }
    }
    return launch_rows(a, nb_for(d->cout), vec, st, pma, models);      // (1 ... 4)
}
