// Training batches from raw scans, behind the voxeliser: the row arrays of both trainers, and the packed symmetry labels.
//
// cv_sp_scan_rows_f32 (joint trainer): the features and the three label arrays of the kept rows of a voxelised batch, computed
// per row from the raw per-vertex arrays - what ScanNetXYZProbMultiDataset.__getitem__ (utils/dataloader.py:118-210) computes
// for EVERY vertex on the host and then gathers by the first-point index.  ONE launch, scan_rows.
//
// Row-array kernels (scan_rows, sym_row_arrays) are laid out like voxel_rows (sparse_coords.hip, section 7): every output owns
// a range of workgroups that strides over its n * width elements, so adjacent lanes write adjacent destination words.  The
// model table ([n_models] x (12 fp64 + 3 fp32 + 1 int32)) and the colour table ([n_clouds][6] fp64) are a few hundred bytes and
// stay in cache; the per-vertex reads follow `index`, which ascends.  About 100 B per row: the launch is bound by its latency.
//
// cv_sp_sym_rows_f32 (separate-model trainer): packed symmetry labels (data.SymBatch, what cv_sym_loss_* consume) and the
// per-row arrays, from the voxeliser's outputs, the raw per-vertex arrays and the per-model vertex lists - what
// ScanNetXYZProbSymDataset.__getitem__ (utils/dataloader.py:339-476) and data.pack_sym compute on the host.  No count is
// known to the host: every launch is sized by the host's upper bounds and reads N, P, S, T, U from device words.
//
//   sym_flag       candidate q survives iff its vertex is the first point of its voxel; block sums of the flags.  On the way:
//                  first row of every cloud (lower bound of its first vertex in `index`), the row counters zeroed.
//   sym_segments   ONE workgroup: scan of the block sums (second level, SCAN_WIDTH sums per trip), kept count of every
//                  segment, the kept segments renumbered, seg_ptr / pose_ptr / tgt_ptr, P S J T.
//   sym_compact    kept candidate -> point p (ordered: block offset + scan inside the block): rows, pseg, its vertex; the row
//                  counters count (integer atomics).
//   sym_targets    one lane per target word, adjacent lanes adjacent words; the segment by bisection of tgt_ptr.
//   row_sums / row_top / row_emit   two-level scan over the row counters: urow, uptr, U, max_row; counter := first slot.
//   upoint_fill    point p takes a slot of its row (atomic: any order), upoint_sort: one lane per row sorts its slots ascending
//                  (insertion sort, quadratic in the row's multiplicity - see cv_hip.h) - the result is the stable order.
//   sym_row_arrays feats / scale / obj / cls of the N kept rows.
//
// Built with -ffp-contract=off (csrc/build.py STRICT): labels, targets and colours are the expressions of cv_hip.h as written.
#include "cv_common.h"

#include <algorithm>

namespace {

constexpr int BLOCK = 256;                          // threads per workgroup; candidates (and row counters) per first scan level
constexpr int SCAN_WIDTH = 1024;                    // block sums per trip of the one-workgroup second level
constexpr int MAX_BLOCKS = 512;                     // per output of the strided kernels: 131072 threads, then the loops stride
enum { C_P = 0, C_S, C_J, C_T, C_U, C_MAXROW, C_N, C_REJECTED };

// ---- what the two row-array kernels share ------------------------------------------------------------------------------

// four outputs in one launch: output s owns the workgroups [block_begin[s], block_begin[s + 1])
struct RowPartition {
    int block_begin[5];
};

RowPartition partition_rows(const long long (&elems)[4], int min_blocks) {
    RowPartition p;
    int total = 0;
    for (int s = 0; s < 4; ++s) {
        p.block_begin[s] = total;
        total += (int)std::max<long long>(min_blocks, std::min<long long>((elems[s] + BLOCK - 1) / BLOCK, MAX_BLOCKS));
    }
    p.block_begin[4] = total;
    return p;
}

// this thread's output, its first element there and its step
__device__ __forceinline__ int row_output(const RowPartition& p, long long* first, long long* step) {
    int s = 0;
    while (s < 3 && (int)blockIdx.x >= p.block_begin[s + 1]) ++s;
    const int nb = p.block_begin[s + 1] - p.block_begin[s], blk = blockIdx.x - p.block_begin[s];
    *first = (long long)blk * BLOCK + threadIdx.x;
    *step = (long long)nb * BLOCK;
    return s;
}

// the model of a raw vertex: a row of the model table, or -1 (background; also what an owner outside the table reads as)
template <class Desc>
__device__ __forceinline__ int model_of(const Desc& d, int v) {
    const int o = d.d_owner[v];
    return (unsigned)o < (unsigned)d.n_models ? o : -1;
}

// row m[0..3] of a world -> unit cube matrix applied to the point p, in fp64: this order, no fused multiply-add
__device__ __forceinline__ float label_transform(const double* m, const float* p) {
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    return (float)(((m[0] * x + m[1] * y) + m[2] * z) + m[3]);
}

// The two trainers' colours: raw = rgb[v][k], g = the cloud's (gain, shift) row of the colour table or NULL, jitter = jitter[v].
// Joint: c = (float)((double)rgb[v][k] / 255.0); with a colour table, c = (float)((double)c * colour[b][k]),
// c = (float)((double)c + colour[b][3 + k]), c = (float)((double)c + jitter[v]), then clamped to [0, 1] - every step rounds to
// fp32, as numpy's in-place `float32 op= float64` does.
__device__ __forceinline__ float colour_joint(unsigned char raw, const double* g, int k, double jitter) {
    float x = (float)((double)raw / 255.0);
    if (g) {
        x = (float)((double)x * g[k]);
        x = (float)((double)x + g[3 + k]);
        x = (float)((double)x + jitter);
        x = fminf(fmaxf(x, 0.0f), 1.0f);
    }
    return x;
}

// Separate: without a table c = (float)((double)rgb[v][k] / 255.0); with one, t = (double)rgb[v][k]; t = t * gain[b][k];
// t = t + shift[b][k]; t = t + jitter[v]; t = min(max(t, 0), 1); c = (float)(t / 255.0) - fp64 throughout, one rounding.
__device__ __forceinline__ float colour_separate(unsigned char raw, const double* g, int k, double jitter) {
    double t = (double)raw;
    if (g) {
        t = t * g[k];
        t = t + g[3 + k];
        t = t + jitter;
        t = fmin(fmax(t, 0.0), 1.0);
    }
    return (float)(t / 255.0);
}

// feats of the n kept rows: fw = 3 colour columns, or 6 with the row's point in front; recentre: colours as c * 2.0f - 1.0f
template <float (*COLOUR)(unsigned char, const double*, int, double), class Desc>
__device__ __forceinline__ void feature_rows(const Desc& d, long long n, int fw, long long first, long long step) {
    const int c0 = fw - 3;                          // colour columns: [c0, fw)
    for (long long e = first; e < n * fw; e += step) {
        const long long i = e / fw;
        const int c = (int)(e - i * fw);
        const long long v = d.d_index[i];
        float x;
        if (c < c0) {
            x = d.d_points[v * d.points_ld + c];
        } else {
            const double* g = nullptr;
            double jitter = 0.0;
            if (d.d_colour) {
                const int b = d.d_coords4[4 * i];
                g = d.d_colour + 6ll * ((unsigned)b < (unsigned)d.n_clouds ? b : 0);
                jitter = d.d_jitter[v];
            }
            x = COLOUR(d.d_rgb[v * 3 + (c - c0)], g, c - c0, jitter);
            if (d.recentre) x = x * 2.0f - 1.0f;
        }
        d.d_feats[i * d.feats_ld + c] = x;
    }
}

// scale of the n kept rows: the model's, background 0
template <class Desc>
__device__ __forceinline__ void scale_rows(const Desc& d, long long n, long long first, long long step) {
    for (long long e = first; e < n * 3; e += step) {
        const long long i = e / 3;
        const int r = (int)(e - i * 3);
        const int o = model_of(d, d.d_index[i]);
        d.d_scale[i * d.scale_ld + r] = o >= 0 ? d.d_model_scale[3ll * o + r] : 0.0f;
    }
}

// class of the n kept rows, widened to int64: the model's, or `background`
template <class Desc>
__device__ __forceinline__ void class_rows(const Desc& d, long long n, long long background, long long ld, long long first,
                                           long long step) {
    for (long long i = first; i < n; i += step) {
        const int o = model_of(d, d.d_index[i]);
        d.d_cls[i * ld] = o >= 0 ? (long long)d.d_model_cls[o] : background;
    }
}

// ---- cv_sp_scan_rows_f32 -----------------------------------------------------------------------------------------------

struct ScanRowsDev {
    cv_scan_rows_desc d;
    int fw;                                         // feature width: 3, or 6 with use_xyz
    RowPartition part;                              // feats, xyz, scale, cls
};

__global__ __launch_bounds__(BLOCK) void scan_rows(const ScanRowsDev a) {
    const cv_scan_rows_desc& d = a.d;
    long long first, step;
    const int s = row_output(a.part, &first, &step);
    if (s == 0) {
        feature_rows<colour_joint>(d, d.n, a.fw, first, step);
    } else if (s == 1) {
        for (long long e = first; e < d.n * 3; e += step) {
            const long long i = e / 3;
            const int r = (int)(e - i * 3);
            const long long v = d.d_index[i];
            const int o = model_of(d, (int)v);
            d.d_xyz[i * d.xyz_ld + r] = o >= 0 ? label_transform(d.d_minv + 12ll * o + 4 * r, d.d_points + v * d.points_ld) : 0.0f;
        }
    } else if (s == 2) {
        scale_rows(d, d.n, first, step);
    } else {
        class_rows(d, d.n, 9, d.cls_ld, first, step);                    // background 9: utils/dataloader.py:166
    }
}

// ---- cv_sp_sym_rows_f32 ------------------------------------------------------------------------------------------------

struct SymWs {
    int* flag;        // [Q]
    int* bsum;        // [nblk(Q) + 1]   block sums of the flags -> exclusive
    int* posb;        // [S0 + 1]        kept candidates in front of every segment's list
    int* new_id;      // [S0]            new number of a segment, -1 dropped
    int* job0;        // [S0]            first job (row of minv) of a KEPT segment, by its new number
    int* kept_v;      // [Q]             vertex of kept point p
    int* first_row;   // [n_clouds]
    int* cnt;         // [M]             points per row, then the first free slot of the row
    int* rsum;        // [nblk(M) + 1]   block sums of cnt -> exclusive
    int* usum;        // [nblk(M) + 1]   block sums of (cnt > 0) -> exclusive
};

struct SymDev {
    cv_sym_rows_desc d;
    SymWs w;
    int fw;
    RowPartition part;                              // feats, scale, obj, cls
};

long long nblk(long long n) { return (n + BLOCK - 1) / BLOCK; }

// exclusive scan of one value per thread over the workgroup (blockDim a multiple of 64, every thread calls); sh: 16 ints
__device__ __forceinline__ int block_scan(int x, int* total, int* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int inc = x;
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(inc, d);
        if (lane >= d) inc += y;
    }
    __syncthreads();                                // sh may still be read from the call before
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int off = 0, tot = 0;
    for (int k = 0; k < nw; ++k) {
        const int t = sh[k];
        if (k < w) off += t;
        tot += t;
    }
    *total = tot;
    return off + inc - x;
}

// in place: a[0 .. n) -> its exclusive prefix, a[n] = the total; one workgroup of SCAN_WIDTH threads
__device__ void top_scan(int* a, int n, int* sh) {
    int carry = 0;
    for (int base = 0; base < n; base += SCAN_WIDTH) {
        const int i = base + threadIdx.x;
        const int x = i < n ? a[i] : 0;
        int tot;
        const int ex = block_scan(x, &tot, sh);
        if (i < n) a[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) a[n] = carry;
    __syncthreads();
}

__device__ __forceinline__ int rows_n(const cv_sym_rows_desc& d) {
    const int n = d.d_quant_counts[0];
    return n < 0 ? 0 : (n > (int)d.m_points ? (int)d.m_points : n);
}

// nb: workgroups that hold candidates; the grid may be larger (the extra ones only help to zero the row counters)
__global__ __launch_bounds__(BLOCK) void sym_flag(const SymDev a, int nb) {
    __shared__ int sh[16];
    const cv_sym_rows_desc& d = a.d;
    const int m = (int)d.m_points, n = rows_n(d);
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    int f = 0;
    if (q < d.n_cand) {
        const int v = d.d_seg_vertex[q];
        if ((unsigned)v < (unsigned)m) {
            const int r = d.d_inverse[v];
            f = (unsigned)r < (unsigned)n && d.d_index[r] == v;
        }
        a.w.flag[q] = f;
    }
    int tot;
    block_scan(f, &tot, sh);
    if (threadIdx.x == 0 && (int)blockIdx.x < std::max(nb, 1)) a.w.bsum[blockIdx.x] = tot;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < m; i += (long long)gridDim.x * BLOCK) a.w.cnt[i] = 0;
    if (blockIdx.x == 0)
        for (int b = threadIdx.x; b < d.n_clouds; b += BLOCK) {       // first row r with index[r] >= offsets[b]
            const long long first = d.d_offsets[b];
            int lo = 0, hi = n;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (d.d_index[mid] < first) lo = mid + 1; else hi = mid;
            }
            a.w.first_row[b] = lo;
        }
}

__global__ __launch_bounds__(SCAN_WIDTH) void sym_segments(const SymDev a, int nb) {
    __shared__ int sh[16];
    const cv_sym_rows_desc& d = a.d;
    const SymWs& w = a.w;
    const int S0 = d.n_seg_in;
    top_scan(w.bsum, nb, sh);
    const int Q = (int)d.n_cand;
    for (int s = threadIdx.x; s <= S0; s += SCAN_WIDTH) {                // kept candidates in front of list s
        int q = d.d_seg_vptr[s];
        q = q < 0 ? 0 : (q > Q ? Q : q);
        const int blk = q / BLOCK;
        int p = w.bsum[blk];
        for (int i = blk * BLOCK; i < q; ++i) p += w.flag[i];
        w.posb[s] = p;
    }
    __syncthreads();
    int c_seg = 0, c_len = 0, c_pose = 0, c_tgt = 0;
    for (int base = 0; base < S0; base += SCAN_WIDTH) {
        const int s = base + threadIdx.x;
        int len = 0, np = 0, j0 = 0;
        if (s < S0) {
            len = w.posb[s + 1] - w.posb[s];
            j0 = d.d_seg_pose_ptr[s];
            np = d.d_seg_pose_ptr[s + 1] - j0;
            if (len < 0 || np < 0) len = 0;
        }
        const int keep = len > 0;
        if (!keep) np = 0;
        int t_seg, t_len, t_pose, t_tgt;
        const int e_seg = block_scan(keep, &t_seg, sh), e_len = block_scan(len, &t_len, sh),
                  e_pose = block_scan(np, &t_pose, sh), e_tgt = block_scan(len * np, &t_tgt, sh);
        if (s < S0) w.new_id[s] = keep ? c_seg + e_seg : -1;
        if (keep) {
            const int k = c_seg + e_seg;
            d.d_seg_ptr[k] = c_len + e_len;
            d.d_pose_ptr[k] = c_pose + e_pose;
            d.d_tgt_ptr[k] = c_tgt + e_tgt;
            w.job0[k] = j0;
        }
        c_seg += t_seg; c_len += t_len; c_pose += t_pose; c_tgt += t_tgt;
    }
    if (threadIdx.x == 0) {
        d.d_seg_ptr[c_seg] = c_len;
        d.d_pose_ptr[c_seg] = c_pose;
        d.d_tgt_ptr[c_seg] = c_tgt;
        d.d_counts[C_P] = c_len;
        d.d_counts[C_S] = c_seg;
        d.d_counts[C_J] = c_pose;
        d.d_counts[C_T] = c_tgt;
        d.d_counts[C_N] = d.d_quant_counts[0];
        d.d_counts[C_REJECTED] = d.d_quant_counts[1];
    }
}

__global__ __launch_bounds__(BLOCK) void sym_compact(const SymDev a) {
    __shared__ int sh[16];
    const cv_sym_rows_desc& d = a.d;
    const SymWs& w = a.w;
    const long long q = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const int f = q < d.n_cand ? w.flag[q] : 0;
    int tot;
    const int p = w.bsum[blockIdx.x] + block_scan(f, &tot, sh);
    if (!f) return;
    int lo = 0, hi = d.n_seg_in - 1;                                      // last list that starts at or before q
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (d.d_seg_vptr[mid] <= q) lo = mid; else hi = mid - 1;
    }
    const int v = d.d_seg_vertex[q], r = d.d_inverse[v];
    int row = r;
    if (d.reference_indexing) {
        const int b = d.d_coords4[4ll * r];
        row = r - w.first_row[(unsigned)b < (unsigned)d.n_clouds ? b : 0];
    }
    d.d_rows[p] = row;
    d.d_pseg[p] = w.new_id[lo];
    w.kept_v[p] = v;
    if ((unsigned)row < (unsigned)d.m_points) atomicAdd(&w.cnt[row], 1);
}

__global__ __launch_bounds__(BLOCK) void sym_targets(const SymDev a) {
    const cv_sym_rows_desc& d = a.d;
    const SymWs& w = a.w;
    const int S = d.d_counts[C_S];
    const long long words = 3 * std::min<long long>(d.d_counts[C_T], d.n_targets_in);
    for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < words; e += (long long)gridDim.x * BLOCK) {
        const int t = (int)(e / 3), r = (int)(e - 3ll * t);
        int lo = 0, hi = S - 1;                                           // last kept segment whose block starts at or before t
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (d.d_tgt_ptr[mid] <= t) lo = mid; else hi = mid - 1;
        }
        const int p0 = d.d_seg_ptr[lo], len = d.d_seg_ptr[lo + 1] - p0;
        const int k = t - d.d_tgt_ptr[lo], j = k / len, i = k - j * len;
        long long job = (long long)w.job0[lo] + j;
        job = job < 0 ? 0 : (job >= d.n_jobs_in ? d.n_jobs_in - 1 : job);
        d.d_targets[e] = label_transform(d.d_minv + 12 * job + 4 * r, d.d_points + (long long)w.kept_v[p0 + i] * d.points_ld);
    }
}

__global__ __launch_bounds__(BLOCK) void row_sums(const SymDev a) {
    __shared__ int sh[16];
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const int c = i < a.d.m_points ? a.w.cnt[i] : 0;
    int tot, utot;
    block_scan(c, &tot, sh);
    block_scan(c > 0, &utot, sh);
    if (threadIdx.x == 0) {
        a.w.rsum[blockIdx.x] = tot;
        a.w.usum[blockIdx.x] = utot;
    }
}

__global__ __launch_bounds__(SCAN_WIDTH) void row_top(const SymDev a, int nb) {
    __shared__ int sh[16];
    top_scan(a.w.rsum, nb, sh);
    top_scan(a.w.usum, nb, sh);
    if (threadIdx.x == 0) {
        const int U = a.w.usum[nb];
        a.d.d_counts[C_U] = U;
        a.d.d_uptr[U] = a.w.rsum[nb];
        if (U == 0) a.d.d_counts[C_MAXROW] = -1;
    }
}

__global__ __launch_bounds__(BLOCK) void row_emit(const SymDev a, int nb) {
    __shared__ int sh[16];
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const int c = i < a.d.m_points ? a.w.cnt[i] : 0;
    int tot;
    const int start = a.w.rsum[blockIdx.x] + block_scan(c, &tot, sh);
    const int u = a.w.usum[blockIdx.x] + block_scan(c > 0, &tot, sh);
    if (c > 0) {
        a.d.d_urow[u] = (int)i;
        a.d.d_uptr[u] = start;
        a.w.cnt[i] = start;                                               // the row's first free slot
        if (u == a.w.usum[nb] - 1) a.d.d_counts[C_MAXROW] = (int)i;
    }
}

__global__ __launch_bounds__(BLOCK) void upoint_fill(const SymDev a) {
    const cv_sym_rows_desc& d = a.d;
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= d.d_counts[C_P]) return;
    const int row = d.d_rows[p];
    if ((unsigned)row < (unsigned)d.m_points) d.d_upoint[atomicAdd(&a.w.cnt[row], 1)] = p;
}

__global__ __launch_bounds__(BLOCK) void upoint_sort(const SymDev a) {
    const cv_sym_rows_desc& d = a.d;
    const int U = d.d_counts[C_U];
    for (int u = blockIdx.x * BLOCK + threadIdx.x; u < U; u += gridDim.x * BLOCK) {
        const int b = d.d_uptr[u], e = d.d_uptr[u + 1];
        for (int i = b + 1; i < e; ++i) {
            const int key = d.d_upoint[i];
            int k = i - 1;
            while (k >= b && d.d_upoint[k] > key) {
                d.d_upoint[k + 1] = d.d_upoint[k];
                --k;
            }
            d.d_upoint[k + 1] = key;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void sym_row_arrays(const SymDev a) {
    const cv_sym_rows_desc& d = a.d;
    const long long n = rows_n(d);
    long long first, step;
    const int s = row_output(a.part, &first, &step);
    if (s == 0) {
        feature_rows<colour_separate>(d, n, a.fw, first, step);
    } else if (s == 1) {
        scale_rows(d, n, first, step);
    } else if (s == 2) {
        for (long long i = first; i < n; i += step) d.d_obj[i] = model_of(d, d.d_index[i]) >= 0;
    } else {
        class_rows(d, n, 0, 1, first, step);                             // background (and 'others') 0
    }
}

SymWs carve(void* ws, long long m, long long q, int s0, int n_clouds, size_t* bytes) {
    CvCarver cv(ws);
    SymWs w;
    w.flag = cv.take<int>((size_t)q);
    w.bsum = cv.take<int>((size_t)nblk(q) + 2);
    w.posb = cv.take<int>((size_t)s0 + 1);
    w.new_id = cv.take<int>((size_t)s0 + 1);
    w.job0 = cv.take<int>((size_t)s0 + 1);
    w.kept_v = cv.take<int>((size_t)q);
    w.first_row = cv.take<int>((size_t)n_clouds);
    w.cnt = cv.take<int>((size_t)m);
    w.rsum = cv.take<int>((size_t)nblk(m) + 1);
    w.usum = cv.take<int>((size_t)nblk(m) + 1);
    *bytes = cv_align_up(cv.off, 256);
    return w;
}

int strided_blocks(long long elems) { return (int)std::max<long long>(1, std::min<long long>(nblk(elems), MAX_BLOCKS)); }

}  // namespace

extern "C" {

int cv_sp_scan_rows_f32(const cv_scan_rows_desc* desc, void* stream) {
    CV_REQUIRE(desc, CV_EINVAL, "null scan-rows descriptor");
    const cv_scan_rows_desc& d = *desc;
    CV_REQUIRE(d.n > 0 && d.n <= (1ll << 29), CV_EINVAL, "bad row count %lld", d.n);
    CV_REQUIRE(d.m_points > 0 && d.m_points <= (1ll << 29), CV_EINVAL, "bad point count %lld", d.m_points);
    CV_REQUIRE(d.n <= d.m_points, CV_EINVAL, "more kept rows (%lld) than points (%lld)", d.n, d.m_points);
    CV_REQUIRE(d.n_models >= 0, CV_EINVAL, "bad model count %d", d.n_models);
    CV_REQUIRE(d.n_clouds >= 1, CV_EINVAL, "bad cloud count %d", d.n_clouds);
    CV_REQUIRE(d.d_coords4 && d.d_index && d.d_points && d.d_rgb && d.d_owner && d.d_feats && d.d_xyz && d.d_scale && d.d_cls,
               CV_EINVAL, "null pointer argument");
    CV_REQUIRE(d.n_models == 0 || (d.d_minv && d.d_model_scale && d.d_model_cls), CV_EINVAL,
               "null pointer argument (model table of %d rows)", d.n_models);
    CV_REQUIRE(!d.d_jitter || d.d_colour, CV_EINVAL, "jitter without a colour table");
    CV_REQUIRE(!d.d_colour || d.d_jitter, CV_EINVAL, "colour table without jitter");
    const int fw = d.use_xyz ? 6 : 3;
    CV_REQUIRE(d.points_ld >= 3, CV_EINVAL, "row stride %lld of the points below 3", d.points_ld);
    CV_REQUIRE(d.feats_ld >= fw && d.xyz_ld >= 3 && d.scale_ld >= 3 && d.cls_ld >= 1, CV_EINVAL,
               "destination row stride below its width (feats %lld < %d, xyz %lld, scale %lld < 3, or cls %lld < 1)",
               d.feats_ld, fw, d.xyz_ld, d.scale_ld, d.cls_ld);
    ScanRowsDev a = {};
    a.d = d;
    a.fw = fw;
    a.part = partition_rows({d.n * fw, d.n * 3, d.n * 3, d.n}, 0);
    scan_rows<<<a.part.block_begin[4], BLOCK, 0, static_cast<hipStream_t>(stream)>>>(a);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

size_t cv_sizeof_scan_rows_desc(void) { return sizeof(cv_scan_rows_desc); }

size_t cv_sp_sym_rows_workspace_bytes(long long m_points, long long n_cand, int n_seg_in, int n_clouds) {
    if (m_points <= 0 || n_cand < 0 || n_seg_in < 0 || n_clouds < 1) return 0;
    size_t bytes;
    carve(nullptr, m_points, n_cand, n_seg_in, n_clouds, &bytes);
    return bytes;
}

int cv_sp_sym_rows_block(void) { return BLOCK; }
long long cv_sp_sym_rows_scan_span(void) { return (long long)BLOCK * SCAN_WIDTH; }
size_t cv_sizeof_sym_rows_desc(void) { return sizeof(cv_sym_rows_desc); }

int cv_sp_sym_rows_f32(const cv_sym_rows_desc* desc, void* stream) {
    CV_REQUIRE(desc, CV_EINVAL, "null sym-rows descriptor");
    const cv_sym_rows_desc& d = *desc;
    CV_REQUIRE(d.m_points > 0 && d.m_points <= (1ll << 29), CV_EINVAL, "bad point count %lld", d.m_points);
    CV_REQUIRE(d.n_cand >= 0 && d.n_cand <= (1ll << 30), CV_EINVAL, "bad candidate count %lld", d.n_cand);
    CV_REQUIRE(d.n_seg_in >= 0, CV_EINVAL, "bad segment count %d", d.n_seg_in);
    CV_REQUIRE(d.n_jobs_in >= 0 && d.n_jobs_in <= 0x7fffffffll, CV_EINVAL, "bad job count %lld", d.n_jobs_in);
    CV_REQUIRE(d.n_targets_in >= 0 && d.n_targets_in <= 0x7fffffffll, CV_EINVAL, "bad target count %lld", d.n_targets_in);
    CV_REQUIRE(d.n_models >= 0, CV_EINVAL, "bad model count %d", d.n_models);
    CV_REQUIRE(d.n_clouds >= 1 && d.n_clouds <= CV_QUANTIZE_MAX_CLOUDS, CV_EINVAL, "bad cloud count %d", d.n_clouds);
    CV_REQUIRE(d.n_cand == 0 || (d.n_seg_in > 0 && d.n_jobs_in > 0), CV_EINVAL,
               "%lld candidates without segments or poses (%d, %lld)", d.n_cand, d.n_seg_in, d.n_jobs_in);
    CV_REQUIRE(d.d_coords4 && d.d_index && d.d_inverse && d.d_quant_counts && d.d_points && d.d_rgb && d.d_owner && d.d_offsets &&
                   d.d_seg_vptr && d.d_seg_pose_ptr && d.d_seg_ptr && d.d_pose_ptr && d.d_tgt_ptr && d.d_uptr && d.d_feats &&
                   d.d_scale && d.d_obj && d.d_cls && d.d_counts && d.d_ws,
               CV_EINVAL, "null pointer argument");
    CV_REQUIRE(d.n_models == 0 || (d.d_model_scale && d.d_model_cls), CV_EINVAL, "null pointer argument (model table of %d rows)",
               d.n_models);
    CV_REQUIRE(d.n_cand == 0 || (d.d_seg_vertex && d.d_rows && d.d_pseg && d.d_urow && d.d_upoint && d.d_minv), CV_EINVAL,
               "null pointer argument (arrays of %lld candidates)", d.n_cand);
    CV_REQUIRE(d.n_targets_in == 0 || d.d_targets, CV_EINVAL, "null pointer argument (%lld targets)", d.n_targets_in);
    CV_REQUIRE(d.n_cand == 0 || d.n_targets_in >= d.n_cand, CV_EINVAL, "target bound %lld below the %lld candidates",
               d.n_targets_in, d.n_cand);
    CV_REQUIRE(!d.d_jitter || d.d_colour, CV_EINVAL, "jitter without a colour table");
    CV_REQUIRE(!d.d_colour || d.d_jitter, CV_EINVAL, "colour table without jitter");
    const int fw = d.use_xyz ? 6 : 3;
    CV_REQUIRE(d.points_ld >= 3, CV_EINVAL, "row stride %lld of the points below 3", d.points_ld);
    CV_REQUIRE(d.feats_ld >= fw && d.scale_ld >= 3, CV_EINVAL, "destination row stride below its width (feats %lld < %d or scale %lld < 3)",
               d.feats_ld, fw, d.scale_ld);
    size_t need;
    SymDev a = {};
    a.d = d;
    a.w = carve(d.d_ws, d.m_points, d.n_cand, d.n_seg_in, d.n_clouds, &need);
    CV_REQUIRE(d.ws_bytes >= need, CV_ENOMEM, "workspace too small: %zu bytes, %zu needed", d.ws_bytes, need);
    a.fw = fw;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nbq = (int)nblk(d.n_cand), nbm = (int)nblk(d.m_points);

    sym_flag<<<std::max(std::max(nbq, 1), std::min(nbm, MAX_BLOCKS)), BLOCK, 0, st>>>(a, nbq);
    CV_LAUNCH_CHECK();
    sym_segments<<<1, SCAN_WIDTH, 0, st>>>(a, nbq);
    CV_LAUNCH_CHECK();
    if (nbq > 0) {
        sym_compact<<<nbq, BLOCK, 0, st>>>(a);
        CV_LAUNCH_CHECK();
    }
    if (d.n_targets_in > 0 && d.n_cand > 0) {
        sym_targets<<<(int)std::min<long long>(nblk(3 * d.n_targets_in), 8 * MAX_BLOCKS), BLOCK, 0, st>>>(a);
        CV_LAUNCH_CHECK();
    }
    row_sums<<<nbm, BLOCK, 0, st>>>(a);
    CV_LAUNCH_CHECK();
    row_top<<<1, SCAN_WIDTH, 0, st>>>(a, nbm);
    CV_LAUNCH_CHECK();
    row_emit<<<nbm, BLOCK, 0, st>>>(a, nbm);
    CV_LAUNCH_CHECK();
    if (nbq > 0) {
        upoint_fill<<<nbq, BLOCK, 0, st>>>(a);
        CV_LAUNCH_CHECK();
        upoint_sort<<<strided_blocks(std::min(d.n_cand, d.m_points)), BLOCK, 0, st>>>(a);
        CV_LAUNCH_CHECK();
    }
    a.part = partition_rows({d.m_points * fw, d.m_points * 3, d.m_points, d.m_points}, 1);
    sym_row_arrays<<<a.part.block_begin[4], BLOCK, 0, st>>>(a);
    CV_LAUNCH_CHECK();
    if (d.h_counts) CV_HIP_CHECK(hipMemcpyAsync(d.h_counts, d.d_counts, sizeof(int32_t) * 8, hipMemcpyDeviceToHost, st));
    return CV_OK;
}

}  // extern "C"
