// conv_rows: the sparse convolution on fp32 activations with exact fp32 products (v_mfma_f32_32x32x2_f32) - the kernel for
// every shape the piece-product kernels do not take - with its launcher.  When it runs is decided in sparse_conv.hip.
//
// Kernel shape (flavour "rows"): one workgroup = 4 waves owns 128 output rows x (NB*32) output
// channels.  Per kernel offset j it pulls the 128 neighbour indices; if no row of the tile has
// that neighbour the whole offset is skipped (tile-level sparsity).  Otherwise, per 32-channel
// K chunk: gathered input rows (A, 128x32) and the weight slab (B, 32 x NB*32) are staged in
// LDS (next chunk's global loads are issued into registers before the MFMAs of the current
// one), each wave runs 16 k-steps x NB MFMAs on its 32 rows.  The epilogue applies the folded
// BatchNorm/bias affine, the residual and ReLU and stores once.
#include "cv_common.h"

#include <algorithm>

#include "sparse_conv_common.h"

using namespace cvsc;

namespace {

// VEC: Cin % 32 == 0 (float4 gathers inside one offset).  !VEC: flattened K = K*Cin (stem, Cin=3).
template <int NB, bool VEC>
__global__ __launch_bounds__(THREADS) void conv_rows(ConvArgs a) {
    __shared__ float A_s[KC][A_LD];
    __shared__ float B_s[KC][NB * 32];
    __shared__ int nbr_s[TM];
    __shared__ int rows_s[TM];
    __shared__ __attribute__((aligned(16))) float ep_s[4][32][EP_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.y * (NB * 32);

    if (tid < TM) {
        const long long t = tile_of(a) * TM + tid;
        const int* perm = a.row_perm ? a.row_perm + (a.perm_per_split ? (long long)blockIdx.z * a.n_out : 0) : nullptr;
        rows_s[tid] = t < a.n_out ? (perm ? perm[t] : (int)t) : -1;
    }
    __syncthreads();

    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;

    auto compute = [&]() {
#pragma unroll
        for (int kk = 0; kk < KC; kk += 2) {
            const float av = A_s[kk + (lane >> 5)][wave * 32 + (lane & 31)];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const float bv = B_s[kk + (lane >> 5)][nb * 32 + (lane & 31)];
                acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[nb], 0, 0, 0);
            }
        }
    };

    const int nj = a.j_end - a.j_begin;
    if (VEC) {
        // thread -> (row = tid/8 + 32*i, 4 channels at (tid%8)*4) : 8 lanes cover one 128 B row chunk
        const int a_col = (tid & 7) * 4;
        const int a_row = tid >> 3;                      // + 32*i, i = 0..3
        constexpr int B_F4 = KC * NB * 32 / 4;           // float4s in the weight slab
        constexpr int B_PER = (B_F4 + THREADS - 1) / THREADS;
        // work units = (kernel offset, 32-channel chunk); a split owns a contiguous range of units,
        // or a whole offset group when every group has its own row order
        const int nch = a.cin / KC;
        int u_lo, u_hi;
        if (a.perm_per_split) {
            u_lo = (int)((long long)nj * blockIdx.z / a.splits) * nch;
            u_hi = (int)((long long)nj * (blockIdx.z + 1) / a.splits) * nch;
        } else {
            u_lo = (int)((long long)nj * nch * blockIdx.z / a.splits);
            u_hi = (int)((long long)nj * nch * (blockIdx.z + 1) / a.splits);
        }
        const int j_first = a.j_begin + u_lo / nch, j_last = a.j_begin + (u_hi - 1) / nch;
        for (int j = j_first; j <= j_last && u_hi > u_lo; ++j) {
            const int kc_begin = (j == j_first ? u_lo % nch : 0) * KC;
            const int kc_end = (j == j_last ? (u_hi - 1) % nch + 1 : nch) * KC;
            int my = -1;
            if (tid < TM) {
                const int row = rows_s[tid];
                if (row >= 0) {
                    // mask-sorted orders visit the rows at random: the group's map rows were copied in processing
                    // order next to the order itself, so this is a coalesced read (the row-indexed form costs a
                    // 64-byte sector per 4-byte entry: 140 MB per ts1 conv, 35 % of its wave time)
                    if (a.nbr_perm) {
                        const long long tile_id = (long long)gridDim.x - 1 - blockIdx.x;
                        my = a.nbr_perm[((long long)blockIdx.z * a.n_out + tile_id * TM + tid) * a.nbr_perm_w +
                                        (j - (a.j_begin + (int)((long long)nj * blockIdx.z / a.splits)))];
                    } else
                        my = a.nbr ? a.nbr[(long long)row * a.K + j] : row;
                }
                nbr_s[tid] = my;
            }
            if (!__syncthreads_or(my >= 0)) continue;    // nobody in the tile has this neighbour
            // a wave whose 32 rows all miss this neighbour skips its MFMAs; it still takes part in
            // the staging and the barriers.  Rows are processed in an order that groups equal
            // neighbour masks (row_perm), which is what makes whole waves / tiles skippable.
            const bool wave_live = __any(nbr_s[wave * 32 + (lane & 31)] >= 0);
            float4 ra[4], rb[B_PER];
            auto load = [&](int kc) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int src = nbr_s[a_row + 32 * i];
                    ra[i] = src >= 0 ? *reinterpret_cast<const float4*>(a.in + (long long)src * a.in_ld + kc + a_col)
                                     : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int i = 0; i < B_PER; ++i) {
                    const int f = tid + i * THREADS;
                    if (f < B_F4) {
                        const int kr = f / (NB * 8), c4 = (f % (NB * 8)) * 4;
                        const int col = n0 + c4;
                        const float* wp = a.w + ((long long)j * a.cin + kc + kr) * a.cout + col;
                        if (col + 3 < a.cout) rb[i] = *reinterpret_cast<const float4*>(wp);
                        else {
                            rb[i].x = col < a.cout ? wp[0] : 0.f;
                            rb[i].y = col + 1 < a.cout ? wp[1] : 0.f;
                            rb[i].z = col + 2 < a.cout ? wp[2] : 0.f;
                            rb[i].w = 0.f;
                        }
                    }
                }
            };
            auto stage = [&]() {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = a_row + 32 * i;
                    A_s[a_col + 0][r] = ra[i].x; A_s[a_col + 1][r] = ra[i].y;
                    A_s[a_col + 2][r] = ra[i].z; A_s[a_col + 3][r] = ra[i].w;
                }
#pragma unroll
                for (int i = 0; i < B_PER; ++i) {
                    const int f = tid + i * THREADS;
                    if (f < B_F4) {
                        const int kr = f / (NB * 8), c4 = (f % (NB * 8)) * 4;
                        *reinterpret_cast<float4*>(&B_s[kr][c4]) = rb[i];
                    }
                }
            };
            load(kc_begin);
            for (int kc = kc_begin; kc < kc_end; kc += KC) {
                __syncthreads();                 // previous chunk's MFMAs are done with the LDS tiles
                stage();
                __syncthreads();
                if (kc + KC < kc_end) load(kc + KC);  // in flight while the matrix cores run
                if (wave_live) compute();
            }
            __syncthreads();
        }
    } else {
        const int k0 = a.j_begin * a.cin, ktot = a.j_end * a.cin;
        const int nchunks = (ktot - k0 + KC - 1) / KC;
        const int c_lo = (int)((long long)nchunks * blockIdx.z / a.splits);
        const int c_hi = (int)((long long)nchunks * (blockIdx.z + 1) / a.splits);
        for (int kc = k0 + c_lo * KC; kc < k0 + c_hi * KC; kc += KC) {
            __syncthreads();
            for (int e = tid; e < KC * TM; e += THREADS) {
                const int kk = e / TM, r = e % TM;
                const int kf = kc + kk;
                float v = 0.f;
                const int row = rows_s[r];
                if (kf < ktot && row >= 0) {
                    const int j = kf / a.cin, c = kf - j * a.cin;
                    const int src = a.nbr ? a.nbr[(long long)row * a.K + j] : row;
                    if (src >= 0) v = a.in[(long long)src * a.in_ld + c];
                }
                A_s[kk][r] = v;
            }
            for (int e = tid; e < KC * NB * 32; e += THREADS) {
                const int kr = e / (NB * 32), c = e % (NB * 32);
                const int kf = kc + kr, col = n0 + c;
                B_s[kr][c] = (kf < ktot && col < a.cout) ? a.w[(long long)kf * a.cout + col] : 0.f;
            }
            __syncthreads();
            compute();
        }
    }
    if (a.wide) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
            epilogue_store_wide(a, acc[nb], rows_s + wave * 32, n0 + nb * 32, lane, ep_s[wave]);
    } else {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
            epilogue_store(a, acc[nb], rows_s + wave * 32, n0 + nb * 32 + (lane & 31), lane);
    }
}

}  // namespace

void cvsc::launch_conv_rows(const ConvArgs& a, int nb, bool vec, dim3 grid, hipStream_t st) {
    with_nb<4>(nb, [&](auto nbc) {
        constexpr int NB = decltype(nbc)::value;
        if (vec) conv_rows<NB, true><<<grid, THREADS, 0, st>>>(a);
        else conv_rows<NB, false><<<grid, THREADS, 0, st>>>(a);
    });
}
