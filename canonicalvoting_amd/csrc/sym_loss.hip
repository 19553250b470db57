// Coordinate loss of the per-category model over packed symmetry labels (cv_sym_loss_fwd_f32 / cv_sym_loss_bwd_f32):
// per segment (one aligned model) the weighted mean square distance between its rows' predictions and their targets under
// every symmetry-equivalent pose, the MINIMUM over the poses, the mean over the segments (train_separate.py:265-280) - and
// the gradient of that through the winning pose.  Layout of the labels: cv_sym_loss_desc in cv_hip.h.
//
// Forward, two launches.
//   sym_pose_partials  one workgroup per (segment, chunk of SYM_CHUNK rows).  The chunk is walked as 3 * SYM_CHUNK ELEMENTS
//                      (row-major x, y, z), lane t owning elements t, t + 256, t + 512: its three predictions are gathered
//                      once (out[row * ld + c]) and stay in registers over all poses of the segment, and a pose's targets
//                      for the chunk are 3 * rows adjacent words read by adjacent lanes.  A term is w_c * (p - x)^2 in fp64
//                      (the difference of two fp32 values is exact there); lane sum in element order, wave sum by a
//                      shuffle tree, workgroup sum wave 0 + 1 + 2 + 3.  One fp64 partial per (pose, chunk).
//   sym_select         ONE workgroup.  Per (segment, pose) job the chunk partials are added in chunk order and divided by
//                      3 * len: pose_loss (fp32).  Per segment the minimum over its poses on those fp32 values, the lowest
//                      pose on ties, NaN wins as in torch.min.  The segment losses are added per lane in segment order
//                      (lane t: t, t + 256, ...) and over the lanes by a fixed tree in LDS: any number of segments.
// Backward, one launch: one lane per distinct labelled row over the row's labelled points in ascending point order.
//
// No atomics; every order of summation depends on the labels and SYM_CHUNK alone, so all outputs are the same bytes on
// every run and stream.  Built with -ffp-contract=off (csrc/build.py STRICT): the expressions are evaluated as written.
//
// Where the partials live without a prefix over chunk counts: with C = SYM_CHUNK, chunk c of segment s is workgroup
//   slot(s, c) = seg_ptr[s] / C + s + c                       (integer division)
// and its partial for pose p lies at
//   word(s, p, c) = tgt_ptr[s] / C + pose_ptr[s] + p * nch + c,      nch = ceil(len / C).
// Both are injective: for a = qC + r and a block of n items of which each takes ceil(len / C) words while advancing the
// pointer by len (n = 1 for slots, n = poses for words), q + n * ceil(len / C) <= (a + n * len) / C + n - the next segment
// starts behind this one's last word.  Slots that no chunk maps to end at once; there are at most P / C + S slots and
// T / C + J words (cv_sym_loss_workspace_bytes).
#include "cv_common.h"

#include <cmath>

namespace {

constexpr int SYM_CHUNK = 256;                    // rows per workgroup of the partial pass
constexpr int SYM_THREADS = 256;

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                                       // lane 0 holds the sum
}

// sum over the workgroup (4 waves) in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* lds4) {
    v = wave_sum(v);
    __syncthreads();                                // lds4 may still be read from the call before
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

__global__ __launch_bounds__(SYM_THREADS) void sym_pose_partials(const cv_sym_loss_desc d, double* partial) {
    __shared__ double lds4[4];
    const int S = d.n_segments;
    const long long w = blockIdx.x;
    // the largest s with seg_ptr[s] / C + s <= w (the key grows strictly with s; key(0) = 0)
    int lo = 0, hi = S - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)(d.d_seg_ptr[mid] / SYM_CHUNK) + mid <= w) lo = mid; else hi = mid - 1;
    }
    const int s = lo;
    const int begin = d.d_seg_ptr[s], len = d.d_seg_ptr[s + 1] - begin;
    const int nch = (len + SYM_CHUNK - 1) / SYM_CHUNK;
    const long long c = w - ((long long)(begin / SYM_CHUNK) + s);
    if (c >= nch) return;                           // a slot between two segments
    const int row0 = (int)c * SYM_CHUNK;            // first row of the chunk inside the segment
    const int elems = 3 * min(SYM_CHUNK, len - row0);
    float pred[3];
    double wc[3];
    for (int k = 0; k < 3; ++k) {
        const int e = threadIdx.x + k * SYM_THREADS;
        pred[k] = 0.0f;
        wc[k] = (double)d.w[e % 3];
        if (e < elems) {
            const long long r = d.d_rows[begin + row0 + e / 3];
            // (rows are in range by the caller's check of max_row; one that is not reads as NaN instead of faulting)
            pred[k] = (r >= 0 && r < d.n_rows) ? d.d_out[r * d.ld + e % 3] : nanf("");
        }
    }
    const int p0 = d.d_pose_ptr[s], n_pose = d.d_pose_ptr[s + 1] - p0;
    const long long word0 = (long long)(d.d_tgt_ptr[s] / SYM_CHUNK) + p0 + c;
    const float* tgt = d.d_targets + 3ll * (d.d_tgt_ptr[s] + row0);
    for (int p = 0; p < n_pose; ++p, tgt += 3ll * len) {
        double acc = 0.0;
        for (int k = 0; k < 3; ++k) {
            const int e = threadIdx.x + k * SYM_THREADS;
            if (e < elems) {
                const double diff = (double)pred[k] - (double)tgt[e];
                acc += wc[k] * (diff * diff);
            }
        }
        const double sum = block_sum(acc, lds4);
        if (threadIdx.x == 0) partial[word0 + (long long)p * nch] = sum;
    }
}

__global__ __launch_bounds__(SYM_THREADS) void sym_select(const cv_sym_loss_desc d, const double* partial) {
    __shared__ double lds[SYM_THREADS];
    const int S = d.n_segments, t = threadIdx.x;
    // (segment, pose) jobs: lane t takes segments t, t + 256, ... and walks their poses
    double mine = 0.0;
    for (int s = t; s < S; s += SYM_THREADS) {
        const int len = d.d_seg_ptr[s + 1] - d.d_seg_ptr[s];
        const int nch = (len + SYM_CHUNK - 1) / SYM_CHUNK;
        const int p0 = d.d_pose_ptr[s], n_pose = d.d_pose_ptr[s + 1] - p0;
        const double* part = partial + (long long)(d.d_tgt_ptr[s] / SYM_CHUNK) + p0;
        float best_v = 0.0f;
        int best_p = 0;
        for (int p = 0; p < n_pose; ++p, part += nch) {
            double sum = 0.0;
            for (int c = 0; c < nch; ++c) sum += part[c];
            const float v = (float)(sum / (3.0 * (double)len));
            d.d_pose_loss[p0 + p] = v;
            // the first pose, a strictly smaller one, or the first NaN (torch.min returns NaN when there is one)
            if (p == 0 || v < best_v || (v != v && best_v == best_v)) {
                best_v = v;
                best_p = p;
            }
        }
        if (n_pose <= 0) best_v = nanf("");         // (the minimum of nothing; the collate never makes such a segment)
        d.d_best[s] = best_p;
        d.d_seg_loss[s] = best_v;
        mine += (double)best_v;
    }
    lds[t] = mine;
    __syncthreads();
    for (int half = SYM_THREADS / 2; half > 0; half >>= 1) {
        if (t < half) lds[t] += lds[t + half];
        __syncthreads();
    }
    if (t == 0) d.d_loss[0] = (float)((double)d.xyz_factor * (lds[0] / (double)S));
}

__global__ __launch_bounds__(SYM_THREADS) void sym_backward(const cv_sym_loss_desc d) {
    const long long u = blockIdx.x * (long long)SYM_THREADS + threadIdx.x;
    if (u >= d.n_urows) return;
    const long long r = d.d_urow[u];
    if (r < 0 || r >= d.n_rows) return;             // (see sym_pose_partials: excluded by the caller's max_row check)
    const double coef = ((double)d.d_grad_loss[0] * (double)d.xyz_factor) * 2.0;
    const double S = (double)d.n_segments;
    double p[3], g[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < 3; ++c) p[c] = (double)d.d_out[r * d.ld + c];
    for (int k = d.d_uptr[u]; k < d.d_uptr[u + 1]; ++k) {
        const int i = d.d_upoint[k];
        const int s = d.d_pseg[i];
        const int begin = d.d_seg_ptr[s], len = d.d_seg_ptr[s + 1] - begin;
        const float* x = d.d_targets + 3ll * (d.d_tgt_ptr[s] + (long long)d.d_best[s] * len + (i - begin));
        const double den = (3.0 * (double)len) * S;
        for (int c = 0; c < 3; ++c) g[c] += ((coef * (double)d.w[c]) * (p[c] - (double)x[c])) / den;
    }
    for (int c = 0; c < 3; ++c) d.d_grad[r * d.grad_ld + c] = (float)g[c];
}

size_t workspace_bytes(long long n_targets, int n_jobs) {
    return ((size_t)(n_targets / SYM_CHUNK) + (size_t)n_jobs + 1) * sizeof(double);
}

int check_labels(const cv_sym_loss_desc& d) {
    CV_REQUIRE(d.n_segments >= 0 && d.n_jobs >= 0 && d.n_points >= 0 && d.n_targets >= 0 && d.n_urows >= 0 && d.n_rows >= 0,
               CV_EINVAL, "negative count (segments %d, jobs %d, points %lld, targets %lld, distinct rows %d, rows %lld)",
               d.n_segments, d.n_jobs, d.n_points, d.n_targets, d.n_urows, d.n_rows);
    CV_REQUIRE(d.n_points < (1ll << 31) && d.n_targets < (1ll << 31), CV_EINVAL,
               "%lld points / %lld targets do not fit the int32 pointers", d.n_points, d.n_targets);
    return CV_OK;
}

}  // namespace

extern "C" {

int cv_sym_loss_chunk_rows(void) { return SYM_CHUNK; }

size_t cv_sizeof_sym_loss_desc(void) { return sizeof(cv_sym_loss_desc); }

size_t cv_sym_loss_workspace_bytes(long long n_targets, int n_jobs) {
    return (n_targets < 0 || n_jobs < 0) ? 0 : workspace_bytes(n_targets, n_jobs);
}

int cv_sym_loss_fwd_f32(const cv_sym_loss_desc* desc, void* stream) {
    CV_REQUIRE(desc, CV_EINVAL, "null sym-loss descriptor");
    const cv_sym_loss_desc& d = *desc;
    if (int rc = check_labels(d)) return rc;
    CV_REQUIRE(d.d_loss, CV_EINVAL, "null pointer argument (loss)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d.n_segments == 0) {
        CV_HIP_CHECK(hipMemsetAsync(d.d_loss, 0, sizeof(float), st));
        return CV_OK;
    }
    CV_REQUIRE(d.d_out && d.d_rows && d.d_seg_ptr && d.d_pose_ptr && d.d_tgt_ptr && d.d_targets && d.d_pose_loss && d.d_best &&
               d.d_seg_loss, CV_EINVAL, "null pointer argument");
    CV_REQUIRE(d.ld >= 3, CV_EINVAL, "row stride %lld of the predictions below 3", d.ld);
    CV_REQUIRE(d.n_jobs >= d.n_segments, CV_EINVAL, "%d jobs for %d segments: every segment has a pose", d.n_jobs, d.n_segments);
    const size_t need = workspace_bytes(d.n_targets, d.n_jobs);
    CV_REQUIRE(d.d_ws && d.ws_bytes >= need, CV_ENOMEM, "sym-loss workspace too small (needs %zu bytes)", need);
    const long long slots = d.n_points / SYM_CHUNK + d.n_segments;
    double* partial = static_cast<double*>(d.d_ws);
    sym_pose_partials<<<(unsigned)slots, SYM_THREADS, 0, st>>>(d, partial);
    CV_LAUNCH_CHECK();
    sym_select<<<1, SYM_THREADS, 0, st>>>(d, partial);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_sym_loss_bwd_f32(const cv_sym_loss_desc* desc, void* stream) {
    CV_REQUIRE(desc, CV_EINVAL, "null sym-loss descriptor");
    const cv_sym_loss_desc& d = *desc;
    if (int rc = check_labels(d)) return rc;
    if (d.n_segments == 0 || d.n_urows == 0) return CV_OK;
    CV_REQUIRE(d.d_out && d.d_pseg && d.d_seg_ptr && d.d_tgt_ptr && d.d_targets && d.d_urow && d.d_uptr && d.d_upoint &&
               d.d_best && d.d_grad_loss && d.d_grad, CV_EINVAL, "null pointer argument");
    CV_REQUIRE(d.ld >= 3 && d.grad_ld >= 3, CV_EINVAL, "row stride below 3 (predictions %lld, gradient %lld)", d.ld, d.grad_ld);
    const unsigned blocks = (unsigned)((d.n_urows + SYM_THREADS - 1) / SYM_THREADS);
    sym_backward<<<blocks, SYM_THREADS, 0, static_cast<hipStream_t>(stream)>>>(d);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

}  // extern "C"
