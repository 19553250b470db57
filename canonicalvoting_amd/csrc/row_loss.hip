// Per-row training losses of both models over the network output (cv_row_loss_fwd_f32 / cv_row_loss_bwd_f32): the masked
// squared errors of the chosen head's coordinate and scale columns and the cross entropy of the logit columns
// (train_joint.py:253-283, its validation form :311-340, train_separate.py:247-262).  Definitions: cv_row_loss_desc in cv_hip.h.
//
// The row is read once.  A lane per row (head_joint) touches both 128-byte lines of a 64-column row for 16 of its 64 words;
// here LPR lanes share a row (16 for the joint layout, 4 where the used columns fit 16 words and the logits 4 lanes) and a
// workgroup stages R = 256 / LPR rows per pass through LDS with adjacent lanes on adjacent words (one 16-byte load per lane
// where base and stride allow it, single words otherwise), in an odd row stride so that the R / 4 rows a wave reads a column
// of fall on different banks.
//
// Forward, two launches.
//   row_loss_partials  one workgroup per chunk of ROW_CHUNK rows, ROW_CHUNK / R passes.  Lane l of a row's group holds logit l:
//                      exp(logit - max) in fp64, the sum by an xor butterfly over the group (every lane the same bits); lanes
//                      0..2 hold component c of both squared errors, added (c0 + c1) + c2.  Lane 0 of group g adds its rows
//                      g, g + R, ... in pass order; the R group sums are added by a halving tree in LDS.  Four fp64 partials
//                      (xyz, scale, ce, object rows) and an int count of labels above the last logit per chunk.
//   row_loss_finish    ONE workgroup: lane t adds the partials of the contiguous stretch [t * per, (t + 1) * per) in order,
//                      per = ceil(chunks / 256), then a halving tree over the 256 lanes; thread 0 divides and rounds.
// Backward, one launch: the same staging and row head (lse recomputed), then lane l of the group writes the quads l, l + LPR,
// ... of the row's gradient columns [0, n_cols) - every element once, zeros included.
//
// No atomics; every order of summation depends on n_rows, the layout and ROW_CHUNK alone.  Built with -ffp-contract=off
// (csrc/build.py STRICT): the expressions are evaluated as written.
#include "cv_common.h"

#include <cmath>

namespace {

constexpr int ROW_CHUNK = 256;                    // rows per workgroup of the partial pass
constexpr int ROW_THREADS = 256;
constexpr int ROW_MAX_LOGITS = 16;
constexpr int ROW_MAX_TILE_WORDS = 8192;          // 16 staged rows: 32 KB of LDS

struct Staging { int n_load, stride, vec; };      // columns staged per row, LDS words per row (odd), 16-byte loads

// rows [row0, row0 + R) x columns [0, n_load) into tile[R][stride]; rows from n_rows on are not read
template <int LPR>
__device__ __forceinline__ void load_tile(const cv_row_loss_desc& d, const Staging s, float* tile, long long row0) {
    constexpr int R = ROW_THREADS / LPR;
    const int t = threadIdx.x;
    if (s.vec) {
        const int q4 = s.n_load >> 2;
        for (int i = t; i < R * q4; i += ROW_THREADS) {
            const int rr = i / q4, c = (i - rr * q4) * 4;
            if (row0 + rr < d.n_rows) {
                const float4 v = *reinterpret_cast<const float4*>(d.d_out + (row0 + rr) * d.ld + c);
                float* p = tile + rr * s.stride + c;
                p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
            }
        }
    } else {
        for (int i = t; i < R * s.n_load; i += ROW_THREADS) {
            const int rr = i / s.n_load, c = i - rr * s.n_load;
            if (row0 + rr < d.n_rows) tile[rr * s.stride + c] = d.d_out[(row0 + rr) * d.ld + c];
        }
    }
}

struct RowHead {
    bool live, obj, bad;        // row inside n_rows; object row; label above the last logit
    int h, tgt;                 // chosen head; cross-entropy target (0 for a bad label, whose terms are NaN)
    float mx;                   // largest logit
    double e, sum;              // exp(logit[l] - mx) of this lane (0 from n_logits on); its sum over the row
};

// what forward and backward share; called by all lanes (the butterfly needs every lane of the group)
template <int LPR>
__device__ __forceinline__ RowHead row_head(const cv_row_loss_desc& d, const float* row, long long r, int l) {
    RowHead s;
    const int L = d.n_logits;
    s.live = r < d.n_rows;
    const long long y = s.live ? (long long)d.d_labels[r] : -1;
    s.obj = s.live && y >= d.obj_lo && y <= d.obj_hi;
    s.bad = s.live && y > L - 1;
    s.tgt = y < 0 ? L - 1 : (s.bad ? 0 : (int)y);
    const float* logit = row + d.logit_col;
    float mx = 0.0f;
    int am = 0;
    if (s.live) {
        mx = logit[0];
        for (int k = 1; k < L; ++k)
            if (logit[k] > mx) { mx = logit[k]; am = k; }
    }
    s.mx = mx;
    s.h = 0;
    if (d.heads > 1) s.h = d.gather == CV_ROW_LOSS_GATHER_ARGMAX ? (am == L - 1 ? 0 : am) : (s.obj ? (int)y : 0);
    s.e = (s.live && l < L) ? exp((double)logit[l] - (double)mx) : 0.0;
    double v = s.e;
    for (int off = LPR / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, LPR);
    s.sum = v;
    return s;
}

__device__ __forceinline__ double weight(const cv_row_loss_desc& d, int c) {
    return (double)(c == 0 ? d.w[0] : (c == 1 ? d.w[1] : d.w[2]));
}

__device__ __forceinline__ double scale_target(const cv_row_loss_desc& d, long long r, int c) {
    const double s = (double)d.d_scale_labels[r * 3 + c];
    return d.log_scale ? log(s) : s;
}

template <int LPR>
__global__ __launch_bounds__(ROW_THREADS) void row_loss_partials(const cv_row_loss_desc d, const Staging st, double* partial,
                                                                  int32_t* bad_partial) {
    constexpr int R = ROW_THREADS / LPR;
    extern __shared__ float tile[];
    __shared__ double red[4][R];
    __shared__ int red_bad[R];
    const int t = threadIdx.x, g = t / LPR, l = t % LPR;
    const long long chunk0 = blockIdx.x * (long long)ROW_CHUNK;
    double a_xyz = 0.0, a_scale = 0.0, a_ce = 0.0, a_cnt = 0.0;
    int a_bad = 0;
    for (int p = 0; p < ROW_CHUNK / R; ++p) {
        const long long row0 = chunk0 + p * R;
        if (row0 >= d.n_rows) break;                // (the same for every lane of the workgroup)
        __syncthreads();                            // the pass before has read its tile
        load_tile<LPR>(d, st, tile, row0);
        __syncthreads();
        const long long r = row0 + g;
        const float* row = tile + g * st.stride;
        const RowHead s = row_head<LPR>(d, row, r, l);
        double ex = 0.0, es = 0.0;
        if (s.obj && l < 3) {                       // background rows: neither prediction nor target is read
            const double wc = weight(d, l);
            if (d.with_xyz) {
                const double diff = (double)row[d.xyz_col + 3 * s.h + l] - (double)d.d_xyz_labels[r * 3 + l];
                ex = wc * (diff * diff);
            }
            const double diff = (double)row[d.scale_col + 3 * s.h + l] - scale_target(d, r, l);
            es = wc * (diff * diff);
        }
        const double e_xyz = (__shfl(ex, 0, LPR) + __shfl(ex, 1, LPR)) + __shfl(ex, 2, LPR);
        const double e_scale = (__shfl(es, 0, LPR) + __shfl(es, 1, LPR)) + __shfl(es, 2, LPR);
        if (l == 0 && s.live) {
            const double picked = s.bad ? (double)nanf("") : (double)row[d.logit_col + s.tgt];
            a_xyz += e_xyz;
            a_scale += e_scale;
            a_ce += ((double)s.mx + log(s.sum)) - picked;
            a_cnt += s.obj ? 1.0 : 0.0;
            a_bad += s.bad ? 1 : 0;
        }
    }
    if (l == 0) {
        red[0][g] = a_xyz; red[1][g] = a_scale; red[2][g] = a_ce; red[3][g] = a_cnt;
        red_bad[g] = a_bad;
    }
    __syncthreads();
    for (int half = R / 2; half > 0; half >>= 1) {
        if (t < half) {
            for (int q = 0; q < 4; ++q) red[q][t] += red[q][t + half];
            red_bad[t] += red_bad[t + half];
        }
        __syncthreads();
    }
    if (t < 4) partial[blockIdx.x * 4ll + t] = red[t][0];
    if (t == 4) bad_partial[blockIdx.x] = red_bad[0];
}

__global__ __launch_bounds__(ROW_THREADS) void row_loss_finish(const cv_row_loss_desc d, const double* partial,
                                                               const int32_t* bad_partial, int chunks) {
    __shared__ double red[4][ROW_THREADS];
    __shared__ int red_bad[ROW_THREADS];
    const int t = threadIdx.x;
    const int per = (chunks + ROW_THREADS - 1) / ROW_THREADS;
    const int b0 = min(t * per, chunks), b1 = min(b0 + per, chunks);
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    for (int b = b0; b < b1; ++b) {
        for (int q = 0; q < 4; ++q) a[q] += partial[b * 4ll + q];
        bad += bad_partial[b];
    }
    for (int q = 0; q < 4; ++q) red[q][t] = a[q];
    red_bad[t] = bad;
    __syncthreads();
    for (int half = ROW_THREADS / 2; half > 0; half >>= 1) {
        if (t < half) {
            for (int q = 0; q < 4; ++q) red[q][t] += red[q][t + half];
            red_bad[t] += red_bad[t + half];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double cnt = red[3][0];
        const double denom = d.empty == CV_ROW_LOSS_EMPTY_NAN ? 3.0 * cnt : fmax(3.0 * cnt, 1.0);
        const float loss_xyz = (float)(((double)d.xyz_factor * red[0][0]) / denom);
        const float loss_scale = (float)(((double)d.scale_factor * red[1][0]) / denom);
        const float loss_class = (float)(red[2][0] / (double)d.n_rows);
        d.d_losses[0] = loss_xyz;
        d.d_losses[1] = loss_scale;
        d.d_losses[2] = loss_class;
        d.d_losses[3] = (loss_scale + loss_xyz) + loss_class;
        d.d_info[0] = (int32_t)cnt;
        d.d_info[1] = red_bad[0];
    }
}

template <int LPR>
__global__ __launch_bounds__(ROW_THREADS) void row_loss_backward(const cv_row_loss_desc d, const Staging st, int grad_vec) {
    constexpr int R = ROW_THREADS / LPR;
    extern __shared__ float tile[];
    __shared__ double e_sh[ROW_THREADS];            // [R][LPR]: exp(logit - max) of every lane
    const int t = threadIdx.x, g = t / LPR, l = t % LPR;
    const int L = d.n_logits;
    const long long chunk0 = blockIdx.x * (long long)ROW_CHUNK;
    const double gl = (double)d.d_grad_loss[0];
    const double cnt = (double)d.d_info[0];
    const double denom = d.empty == CV_ROW_LOSS_EMPTY_NAN ? 3.0 * cnt : fmax(3.0 * cnt, 1.0);
    const double c_xyz = (gl * (double)d.xyz_factor) * 2.0, c_scale = (gl * (double)d.scale_factor) * 2.0;
    const double n = (double)d.n_rows;
    const int quads = (d.n_cols + 3) >> 2;
    for (int p = 0; p < ROW_CHUNK / R; ++p) {
        const long long row0 = chunk0 + p * R;
        if (row0 >= d.n_rows) break;
        __syncthreads();
        load_tile<LPR>(d, st, tile, row0);
        __syncthreads();
        const long long r = row0 + g;
        const float* row = tile + g * st.stride;
        const RowHead s = row_head<LPR>(d, row, r, l);
        e_sh[t] = s.e;
        __syncthreads();
        if (!s.live) continue;
        const int xyz0 = d.xyz_col + 3 * s.h, scale0 = d.scale_col + 3 * s.h;
        float* out = d.d_grad + r * d.grad_ld;
        for (int q = l; q < quads; q += LPR) {
            float v[4];
            for (int j = 0; j < 4; ++j) {
                const int col = 4 * q + j;
                const int k = col - d.logit_col, cs = col - scale0, cx = col - xyz0;
                double val = 0.0;
                if (k >= 0 && k < L) {
                    val = s.bad ? (double)nanf("") : (gl * (e_sh[g * LPR + k] / s.sum - (k == s.tgt ? 1.0 : 0.0))) / n;
                } else if (s.obj && col < d.n_cols) {
                    if (cs >= 0 && cs < 3)
                        val = ((c_scale * weight(d, cs)) * ((double)row[col] - scale_target(d, r, cs))) / denom;
                    else if (d.with_xyz && cx >= 0 && cx < 3)
                        val = ((c_xyz * weight(d, cx)) * ((double)row[col] - (double)d.d_xyz_labels[r * 3 + cx])) / denom;
                }
                v[j] = (float)val;
            }
            if (grad_vec && 4 * q + 3 < d.n_cols) {
                *reinterpret_cast<float4*>(out + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                for (int j = 0; j < 4; ++j)
                    if (4 * q + j < d.n_cols) out[4 * q + j] = v[j];
            }
        }
    }
}

long long chunks_of(long long n_rows) { return (n_rows + ROW_CHUNK - 1) / ROW_CHUNK; }

size_t workspace_bytes(long long n_rows) {
    const size_t chunks = (size_t)(chunks_of(n_rows) > 0 ? chunks_of(n_rows) : 1);
    return chunks * 4 * sizeof(double) + cv_align_up(chunks * sizeof(int32_t), 8);
}

int last_used_col(const cv_row_loss_desc& d) {
    int last = d.logit_col + d.n_logits;
    if (d.scale_col + 3 * d.heads > last) last = d.scale_col + 3 * d.heads;
    if (d.with_xyz && d.xyz_col + 3 * d.heads > last) last = d.xyz_col + 3 * d.heads;
    return last;
}

bool disjoint(int a, int na, int b, int nb) { return a + na <= b || b + nb <= a; }

// 4 lanes per row where the logits fit 4 lanes and the used columns 16 words, else 16
int lanes_per_row(const cv_row_loss_desc& d) { return (d.n_logits <= 4 && last_used_col(d) <= 16) ? 4 : 16; }

int check_desc(const cv_row_loss_desc& d) {
    CV_REQUIRE(d.n_rows >= 0 && d.n_rows < (1ll << 31), CV_EINVAL, "row count %lld outside [0, 2^31)", d.n_rows);
    CV_REQUIRE(d.heads >= 1, CV_EINVAL, "%d heads: at least one", d.heads);
    CV_REQUIRE(d.n_logits >= 2 && d.n_logits <= ROW_MAX_LOGITS, CV_EINVAL, "%d logits outside [2, %d]", d.n_logits, ROW_MAX_LOGITS);
    CV_REQUIRE(d.heads < (1 << 20), CV_EINVAL, "%d heads", d.heads);
    CV_REQUIRE(d.xyz_col >= 0 && d.scale_col >= 0 && d.logit_col >= 0 && d.xyz_col < (1 << 24) && d.scale_col < (1 << 24) &&
               d.logit_col < (1 << 24), CV_EINVAL, "column offset outside [0, 2^24) (xyz %d, scale %d, logits %d)", d.xyz_col,
               d.scale_col, d.logit_col);
    CV_REQUIRE(d.gather == CV_ROW_LOSS_GATHER_LABEL || d.gather == CV_ROW_LOSS_GATHER_ARGMAX, CV_EINVAL, "gather mode %d", d.gather);
    CV_REQUIRE(d.empty == CV_ROW_LOSS_EMPTY_ZERO || d.empty == CV_ROW_LOSS_EMPTY_NAN, CV_EINVAL, "empty mode %d", d.empty);
    if (d.heads > 1) {
        CV_REQUIRE(d.obj_lo >= 0 && d.obj_hi < d.heads, CV_EINVAL, "object labels [%lld, %lld] outside the %d heads", d.obj_lo,
                   d.obj_hi, d.heads);
        CV_REQUIRE(d.gather != CV_ROW_LOSS_GATHER_ARGMAX || d.n_logits - 1 <= d.heads, CV_EINVAL,
                   "argmax over %d logits picks a head beyond the %d heads", d.n_logits, d.heads);
    }
    const int last = last_used_col(d);
    CV_REQUIRE(d.ld >= last, CV_EINVAL, "row stride %lld below the last used column %d", d.ld, last);
    CV_REQUIRE(disjoint(d.scale_col, 3 * d.heads, d.logit_col, d.n_logits) &&
               (!d.with_xyz || (disjoint(d.xyz_col, 3 * d.heads, d.logit_col, d.n_logits) &&
                                disjoint(d.xyz_col, 3 * d.heads, d.scale_col, 3 * d.heads))), CV_EINVAL,
               "overlapping column ranges (xyz %d, scale %d, logits %d, %d heads, %d logits)", d.xyz_col, d.scale_col, d.logit_col,
               d.heads, d.n_logits);
    CV_REQUIRE(16 * ((last + 3) / 4 * 4 + 1) <= ROW_MAX_TILE_WORDS, CV_EINVAL, "%d used columns: 16 staged rows exceed %d words",
               last, ROW_MAX_TILE_WORDS);
    CV_REQUIRE(d.d_info, CV_EINVAL, "null pointer argument (info)");
    if (d.n_rows > 0)
        CV_REQUIRE(d.d_out && d.d_labels && d.d_scale_labels && (d.d_xyz_labels || !d.with_xyz), CV_EINVAL,
                   "null pointer argument (output or labels)");
    return CV_OK;
}

Staging staging_of(const cv_row_loss_desc& d) {
    Staging s;
    const int last = last_used_col(d);
    s.vec = (reinterpret_cast<uintptr_t>(d.d_out) % 16 == 0 && d.ld % 4 == 0 && last % 4 == 0) ? 1 : 0;
    s.n_load = last;                                // nothing behind the last used column is read
    s.stride = s.n_load | 1;
    return s;
}

}  // namespace

extern "C" {

int cv_row_loss_chunk_rows(void) { return ROW_CHUNK; }

size_t cv_sizeof_row_loss_desc(void) { return sizeof(cv_row_loss_desc); }

size_t cv_row_loss_workspace_bytes(long long n_rows) { return n_rows < 0 ? 0 : workspace_bytes(n_rows); }

int cv_row_loss_fwd_f32(const cv_row_loss_desc* desc, void* stream) {
    CV_REQUIRE(desc, CV_EINVAL, "null row-loss descriptor");
    const cv_row_loss_desc& d = *desc;
    if (int rc = check_desc(d)) return rc;
    CV_REQUIRE(d.d_losses, CV_EINVAL, "null pointer argument (losses)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d.n_rows == 0) {
        CV_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d.d_losses),
                                       d.empty == CV_ROW_LOSS_EMPTY_NAN ? 0x7fc00000 : 0, 4, st));
        CV_HIP_CHECK(hipMemsetAsync(d.d_info, 0, 2 * sizeof(int32_t), st));
        return CV_OK;
    }
    const size_t need = workspace_bytes(d.n_rows);
    CV_REQUIRE(d.d_ws && d.ws_bytes >= need, CV_ENOMEM, "row-loss workspace too small (needs %zu bytes)", need);
    const long long chunks = chunks_of(d.n_rows);
    double* partial = static_cast<double*>(d.d_ws);
    int32_t* bad_partial = reinterpret_cast<int32_t*>(partial + 4 * chunks);
    const Staging s = staging_of(d);
    if (lanes_per_row(d) == 4)
        row_loss_partials<4><<<(unsigned)chunks, ROW_THREADS, 64 * s.stride * sizeof(float), st>>>(d, s, partial, bad_partial);
    else
        row_loss_partials<16><<<(unsigned)chunks, ROW_THREADS, 16 * s.stride * sizeof(float), st>>>(d, s, partial, bad_partial);
    CV_LAUNCH_CHECK();
    row_loss_finish<<<1, ROW_THREADS, 0, st>>>(d, partial, bad_partial, (int)chunks);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_row_loss_bwd_f32(const cv_row_loss_desc* desc, void* stream) {
    CV_REQUIRE(desc, CV_EINVAL, "null row-loss descriptor");
    const cv_row_loss_desc& d = *desc;
    if (int rc = check_desc(d)) return rc;
    CV_REQUIRE(d.gather == CV_ROW_LOSS_GATHER_LABEL, CV_EINVAL, "the backward exists for the label gather only");
    const int last = last_used_col(d);
    CV_REQUIRE(d.n_cols >= last && d.grad_ld >= d.n_cols, CV_EINVAL,
               "gradient columns %d below the last used column %d, or row stride %lld below them", d.n_cols, last, d.grad_ld);
    if (d.n_rows == 0) return CV_OK;
    CV_REQUIRE(d.d_grad_loss && d.d_grad, CV_EINVAL, "null pointer argument (gradient)");
    const long long chunks = chunks_of(d.n_rows);
    const Staging s = staging_of(d);
    const int grad_vec = (reinterpret_cast<uintptr_t>(d.d_grad) % 16 == 0 && d.grad_ld % 4 == 0) ? 1 : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (lanes_per_row(d) == 4)
        row_loss_backward<4><<<(unsigned)chunks, ROW_THREADS, 64 * s.stride * sizeof(float), st>>>(d, s, grad_vec);
    else
        row_loss_backward<16><<<(unsigned)chunks, ROW_THREADS, 16 * s.stride * sizeof(float), st>>>(d, s, grad_vec);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

}  // extern "C"
