// The row kernels: everything that walks the rows of an [n][c] feature array without a kernel map, with the C entry points.
//   eval and training: per-channel affine (+ residual, ReLU, hl twin, ReLU bits), bn_fold, fp32 <-> hl, the three heads;
//   training only: column sums (the bias gradient), BatchNorm in training mode (batch statistics, backward) and the
//   guarded copy of an optimiser step (copy_unless_flag).
// tests/test_row_kernels_gpu.py checks them per element against fp64.
#include "cv_common.h"

#include <algorithm>

#include "sparse_conv_common.h"

using namespace cvsc;

namespace {

// ------------------------------------------------------------------ elementwise helpers
// y = x*scale + shift (+relu)   (MinkowskiBatchNorm in eval mode, MinkowskiReLU)
__global__ __launch_bounds__(256) void affine_rows(const float* __restrict__ x, long long n, int c,
                                                   int x_ld, const float* __restrict__ scale,
                                                   const float* __restrict__ shift,
                                                   const float* __restrict__ residual, int res_ld, int relu,
                                                   float* __restrict__ y, int y_ld) {
    for (long long t = blockIdx.x * 256ll + threadIdx.x; t < n * c; t += (long long)gridDim.x * 256) {
        const long long r = t / c;
        const int k = (int)(t - r * c);
        float v = x[r * x_ld + k];
        if (scale) v = v * scale[k] + (shift ? shift[k] : 0.f);
        if (residual) v += residual[r * res_ld + k];
        if (relu) v = fmaxf(v, 0.f);
        y[r * y_ld + k] = v;
    }
}

// float4 flavour (c, leading dimensions % 4 == 0, 16-byte aligned bases): one thread = 4 consecutive channels of a row
__global__ __launch_bounds__(256) void affine_rows4(const float* __restrict__ x, long long n, int c,
                                                    int x_ld, const float* __restrict__ scale,
                                                    const float* __restrict__ shift,
                                                    const float* __restrict__ residual, int res_ld, int relu,
                                                    float* __restrict__ y, int y_ld, float* __restrict__ y_hl = nullptr,
                                                    int y_hl_ld = 0, int* __restrict__ range_flag = nullptr,
                                                    unsigned* __restrict__ ybits = nullptr) {
    const int cq = c >> 2;
    for (long long t = blockIdx.x * 256ll + threadIdx.x; t < n * cq; t += (long long)gridDim.x * 256) {
        const long long r = t / cq;
        const int k = (int)(t - r * cq) * 4;
        float4 v = *reinterpret_cast<const float4*>(x + r * x_ld + k);
        if (scale) {
            const float4 sc = *reinterpret_cast<const float4*>(scale + k);
            const float4 sh = shift ? *reinterpret_cast<const float4*>(shift + k) : make_float4(0.f, 0.f, 0.f, 0.f);
            v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
        }
        if (residual) {
            const float4 p = *reinterpret_cast<const float4*>(residual + r * res_ld + k);
            v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        *reinterpret_cast<float4*>(y + r * y_ld + k) = v;
        if (y_hl) {                                  // the same values once more as the fp16 pairs the next convolution multiplies
            if (range_flag && hl_out_of_range(v)) *range_flag = 1;
            hl_store4(y_hl + r * y_hl_ld, k, v);
        }
        if (ybits) {
            // where the ReLU is open, one bit per element: the 8 lanes of a row's 32-channel chunk (c % 32 == 0: they are
            // consecutive lanes of one wave, all active together) OR their nibbles into one word
            unsigned w = ((v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u)) << (k & 31);
            w |= (unsigned)__shfl_xor((int)w, 1);
            w |= (unsigned)__shfl_xor((int)w, 2);
            w |= (unsigned)__shfl_xor((int)w, 4);
            if ((k & 31) == 0) ybits[r * (c >> 5) + (k >> 5)] = w;
        }
    }
}

// scale = gamma * rsqrt(var + eps), shift = beta - mean*scale (+ bias*scale)
__global__ void bn_fold(const float* gamma, const float* beta, const float* mean, const float* var,
                        const float* bias, float eps, int c, float* scale, float* shift) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    const float s = gamma[k] / sqrtf(var[k] + eps);
    scale[k] = s;
    shift[k] = beta[k] - mean[k] * s + (bias ? bias[k] * s : 0.f);
}

// fp32 rows <-> hl format (boundary of the format: tests, modular callers)
__global__ __launch_bounds__(256) void to_hl(const float* __restrict__ x, long long n, int c, int x_ld, float* __restrict__ y,
                                             int y_ld, int* __restrict__ range_flag) {
    const int cq = c >> 2;
    const long long total = n * cq;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long row = e / cq;
        const int col = (int)(e - row * cq) * 4;
        const float* p = x + row * x_ld + col;
        const float4 v = make_float4(p[0], p[1], p[2], p[3]);
        if (range_flag && hl_out_of_range(v)) *range_flag = 1;
        hl_store4(y + row * y_ld, col, v);
    }
}
__global__ __launch_bounds__(256) void from_hl(const float* __restrict__ x, long long n, int c, int x_ld, float* __restrict__ y,
                                               int y_ld) {
    const int cq = c >> 2;
    const long long total = n * cq;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long row = e / cq;
        const int col = (int)(e - row * cq) * 4;
        const float4 v = hl_load4(x + row * x_ld, col);
        float* p = y + row * y_ld + col;
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
}

// eval_joint.py:173-190: per point, head select by argmax class (class 9 -> head 0), exp(scale),
// prob = max softmax over the 9 object classes, class = argmax over the 9 object logits.
__global__ __launch_bounds__(256) void head_joint(const float* __restrict__ f, long long n, int ld,
                                                  int ncls, int log_scale, float* __restrict__ xyz,
                                                  float* __restrict__ scale, float* __restrict__ prob,
                                                  int* __restrict__ cls) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= n) return;
    const float* row = f + i * ld;
    const float* logit = row + 6 * ncls;
    float mx = logit[0];
    int am = 0;
    for (int k = 1; k <= ncls; ++k)
        if (logit[k] > mx) { mx = logit[k]; am = k; }
    float mo = logit[0];
    int ao = 0;
    for (int k = 1; k < ncls; ++k)
        if (logit[k] > mo) { mo = logit[k]; ao = k; }
    float den = 0.f;
    for (int k = 0; k <= ncls; ++k) den += expf(logit[k] - mx);
    const int h = am == ncls ? 0 : am;
    for (int d = 0; d < 3; ++d) {
        xyz[i * 3 + d] = row[h * 3 + d];
        const float s = row[3 * ncls + h * 3 + d];
        scale[i * 3 + d] = log_scale ? expf(s) : s;
    }
    prob[i] = expf(mo - mx) / den;
    cls[i] = ao;
}

// eval_separate.py:170-181 / train_separate.py:247-249,362: 8-channel head of a per-category model:
// xyz = f[0:3], scale = exp(f[3:6]), prob = softmax(f[6:8])[1]
__device__ __forceinline__ void head_separate_row(const float* row, long long i, int log_scale, float* __restrict__ xyz,
                                                  float* __restrict__ scale, float* __restrict__ prob) {
    for (int d = 0; d < 3; ++d) {
        xyz[i * 3 + d] = row[d];
        scale[i * 3 + d] = log_scale ? expf(row[3 + d]) : row[3 + d];
    }
    const float mx = fmaxf(row[6], row[7]);
    const float e0 = expf(row[6] - mx), e1 = expf(row[7] - mx);
    prob[i] = e1 / (e0 + e1);
}
__global__ __launch_bounds__(256) void head_separate(const float* __restrict__ f, long long n, int ld,
                                                     int log_scale, float* __restrict__ xyz,
                                                     float* __restrict__ scale, float* __restrict__ prob) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= n) return;
    head_separate_row(f + i * ld, i, log_scale, xyz, scale, prob);
}

// the same head over the model axis: blockIdx.y = model, outputs [K][n][3], [K][n][3], [K][n]
struct HeadModels { const float* f[CV_MAX_CATEGORIES]; };
__global__ __launch_bounds__(256) void head_separate_models(HeadModels hm, long long n, int ld, int log_scale,
                                                            float* __restrict__ xyz, float* __restrict__ scale,
                                                            float* __restrict__ prob) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= n) return;
    const long long m = blockIdx.y;
    head_separate_row(hm.f[m] + i * ld, i, log_scale, xyz + m * n * 3, scale + m * n * 3, prob + m * n);
}

// ------------------------------------------------------------------ column sums (bias gradient)
// blocks over (32 columns, row chunk).  The block's sum of column blockIdx.x * 32 + (threadIdx.x & 31) over row chunk
// blockIdx.y: eight row lanes, then their sums in lane order; true in the threads that hold a column's sum (t) - what they do
// with it is the caller's
__device__ __forceinline__ bool col_block_sum(const float* __restrict__ x, long long n, int c, int ld, int& col, float& t) {
    __shared__ float s[8][32];
    col = blockIdx.x * 32 + (threadIdx.x & 31);
    const int ry = threadIdx.x >> 5;
    const long long r_lo = n * blockIdx.y / gridDim.y, r_hi = n * (blockIdx.y + 1) / gridDim.y;
    float acc = 0.f;
    if (col < c)
        for (long long r = r_lo + ry; r < r_hi; r += 8) acc += x[r * ld + col];
    s[ry][threadIdx.x & 31] = acc;
    __syncthreads();
    if (!(ry == 0 && col < c)) return false;
    t = 0.f;
    for (int k = 0; k < 8; ++k) t += s[k][threadIdx.x & 31];
    return true;
}
// the partial sums meet through fp32 atomics on the c output words (out is pre-zeroed)
__global__ __launch_bounds__(256) void col_sum(const float* __restrict__ x, long long n, int c, int ld,
                                               float* __restrict__ out) {
    int col;
    float t;
    if (col_block_sum(x, n, c, ld, col, t)) unsafeAtomicAdd(&out[col], t);
}

// the same sums without atomics: every (32 columns, row chunk) block writes its partial sums to ws[chunk][c], a second
// launch adds the chunks of a column in chunk order - the result does not depend on the order in which workgroups run
__global__ __launch_bounds__(256) void col_sum_partial(const float* __restrict__ x, long long n, int c, int ld,
                                                       float* __restrict__ ws) {
    int col;
    float t;
    if (col_block_sum(x, n, c, ld, col, t)) ws[(long long)blockIdx.y * c + col] = t;
}
__global__ __launch_bounds__(256) void col_sum_chunks(const float* __restrict__ ws, int chunks, int c,
                                                      float* __restrict__ out) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= c) return;
    out[col] = sum_in_order4(ws + col, chunks, c);
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

// both affine entry points behind their own first check: d_y_hl (with d_relu_bits, range_flag) is cv_sp_affine_hl_f32's and
// takes the float4 kernel
static int affine_impl(const float* d_x, long long n, int c, int x_ld, const float* d_scale, const float* d_shift,
                       const float* d_residual, int res_ld, int relu, float* d_y, int y_ld, float* d_y_hl, int y_hl_ld,
                       uint32_t* d_relu_bits, int32_t* range_flag, void* stream) {
    CV_REQUIRE(!d_residual || res_ld >= c, CV_EINVAL, "bad residual stride");
    CV_REQUIRE(d_scale || !d_shift, CV_EINVAL, "a shift without a scale is not applied by the kernels");
    const bool v4 = c % 4 == 0 && x_ld % 4 == 0 && y_ld % 4 == 0 && (!d_residual || res_ld % 4 == 0) && aligned16(d_x) &&
                    aligned16(d_y) && aligned16(d_residual) && aligned16(d_scale) && aligned16(d_shift);
    if (d_y_hl) {
        CV_REQUIRE(c % 32 == 0 && y_hl_ld % 32 == 0 && (reinterpret_cast<uintptr_t>(d_y_hl) & 127) == 0, CV_EINVAL,
                   "hl-format output: channels and leading dimension %% 32 == 0, 128-byte aligned rows");
        CV_REQUIRE(v4, CV_EINVAL, "16-byte aligned operands with leading dimensions %% 4 == 0");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (v4)
        affine_rows4<<<(unsigned)std::min<long long>((n * (c / 4) + 255) / 256, 16384), 256, 0, st>>>(
            d_x, n, c, x_ld, d_scale, d_shift, d_residual, res_ld, relu, d_y, y_ld, d_y_hl, y_hl_ld, range_flag, d_relu_bits);
    else
        affine_rows<<<(unsigned)std::min<long long>((n * c + 255) / 256, 8192), 256, 0, st>>>(
            d_x, n, c, x_ld, d_scale, d_shift, d_residual, res_ld, relu, d_y, y_ld);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_sp_affine_f32(const float* d_x, long long n, int c, int x_ld, const float* d_scale,
                     const float* d_shift, const float* d_residual, int res_ld, int relu, float* d_y, int y_ld,
                     void* stream) {
    CV_REQUIRE(d_x && d_y && n > 0 && c > 0 && x_ld >= c && y_ld >= c, CV_EINVAL, "bad affine arguments");
    return affine_impl(d_x, n, c, x_ld, d_scale, d_shift, d_residual, res_ld, relu, d_y, y_ld, nullptr, 0, nullptr, nullptr, stream);
}

int cv_sp_affine_hl_f32(const float* d_x, long long n, int c, int x_ld, const float* d_scale, const float* d_shift,
                        const float* d_residual, int res_ld, int relu, float* d_y, int y_ld, float* d_y_hl, int y_hl_ld,
                        uint32_t* d_relu_bits, int32_t* range_flag, void* stream) {
    CV_REQUIRE(d_x && d_y && d_y_hl && n > 0 && c > 0 && x_ld >= c && y_ld >= c && y_hl_ld >= c, CV_EINVAL, "bad affine arguments");
    return affine_impl(d_x, n, c, x_ld, d_scale, d_shift, d_residual, res_ld, relu, d_y, y_ld, d_y_hl, y_hl_ld, d_relu_bits,
                       range_flag, stream);
}

int cv_sp_to_hl_f32(const float* d_x, long long n, int c, int x_ld, float* d_y, int y_ld, int32_t* range_flag, void* stream) {
    CV_REQUIRE(d_x && d_y && n > 0 && c > 0 && c % 32 == 0 && x_ld >= c && y_ld >= c && y_ld % 32 == 0 &&
                   (reinterpret_cast<uintptr_t>(d_y) & 127) == 0, CV_EINVAL,
               "hl format: channels and leading dimension %% 32 == 0, 128-byte aligned rows");
    to_hl<<<(unsigned)std::min<long long>((n * (c / 4) + 255) / 256, 8192), 256, 0, static_cast<hipStream_t>(stream)>>>(
        d_x, n, c, x_ld, d_y, y_ld, range_flag);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_sp_from_hl_f32(const float* d_x, long long n, int c, int x_ld, float* d_y, int y_ld, void* stream) {
    CV_REQUIRE(d_x && d_y && n > 0 && c > 0 && c % 32 == 0 && x_ld >= c && y_ld >= c && x_ld % 32 == 0 &&
                   (reinterpret_cast<uintptr_t>(d_x) & 127) == 0, CV_EINVAL,
               "hl format: channels and leading dimension %% 32 == 0, 128-byte aligned rows");
    from_hl<<<(unsigned)std::min<long long>((n * (c / 4) + 255) / 256, 8192), 256, 0, static_cast<hipStream_t>(stream)>>>(
        d_x, n, c, x_ld, d_y, y_ld);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_sp_bn_fold_f32(const float* d_gamma, const float* d_beta, const float* d_mean, const float* d_var,
                      const float* d_bias, float eps, int c, float* d_scale, float* d_shift, void* stream) {
    CV_REQUIRE(d_gamma && d_beta && d_mean && d_var && d_scale && d_shift && c > 0, CV_EINVAL, "bad bn_fold arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    bn_fold<<<(c + 127) / 128, 128, 0, st>>>(d_gamma, d_beta, d_mean, d_var, d_bias, eps, c, d_scale, d_shift);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_head_joint_f32(const float* d_feats, long long n, int ld, int nclasses, int log_scale, float* d_xyz,
                      float* d_scale, float* d_prob, int32_t* d_class, void* stream) {
    CV_REQUIRE(d_feats && d_xyz && d_scale && d_prob && d_class, CV_EINVAL, "null pointer argument");
    CV_REQUIRE(n > 0 && nclasses > 0 && nclasses < 64 && ld >= 7 * nclasses + 1, CV_EINVAL, "bad head arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    head_joint<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(d_feats, n, ld, nclasses, log_scale, d_xyz,
                                                           d_scale, d_prob, d_class);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_head_separate_f32(const float* d_feats, long long n, int ld, int log_scale, float* d_xyz, float* d_scale,
                         float* d_prob, void* stream) {
    CV_REQUIRE(d_feats && d_xyz && d_scale && d_prob && n > 0 && ld >= 8, CV_EINVAL, "bad head arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    head_separate<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(d_feats, n, ld, log_scale, d_xyz, d_scale, d_prob);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_head_separate_models_f32(const float* const* d_feats, int K, long long n, int ld, int log_scale, float* d_xyz,
                                float* d_scale, float* d_prob, void* stream) {
    CV_REQUIRE(d_feats && d_xyz && d_scale && d_prob && n > 0 && ld >= 8, CV_EINVAL, "bad head arguments");
    CV_REQUIRE(K >= 1 && K <= CV_MAX_CATEGORIES, CV_EINVAL, "number of models out of range (%d, 1..%d)", K, CV_MAX_CATEGORIES);
    HeadModels hm = {};
    for (int k = 0; k < K; ++k) {
        CV_REQUIRE(d_feats[k], CV_EINVAL, "model %d: null network output", k);
        hm.f[k] = d_feats[k];
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    head_separate_models<<<dim3((unsigned)((n + 255) / 256), (unsigned)K), 256, 0, st>>>(hm, n, ld, log_scale, d_xyz, d_scale, d_prob);
    CV_LAUNCH_CHECK();
    return CV_OK;
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
