// What prepares the operands of a sparse-convolution launch, once per weight tensor or per kernel map: the weight packers
// (bf16 triples, fp16 pairs, one bf16 plane, the stem's layout; pack_weights_*) and the mask orders (mask_keys, mp_*: rows
// sorted by the bit mask of their valid neighbours), with their entry points.
#include "cv_common.h"

#include <algorithm>

#include "sparse_conv_common.h"

using namespace cvsc;

namespace {

// wp layout of the fp16 pairs (unsigned short): ((((j*nch + c)*2 + plane)*cout + col)*32 + k); values are
// w * col_scale * mult (mult = 2^scale_log2 keeps the low pieces of small weights out of the fp16 subnormals)
__global__ __launch_bounds__(256) void pack_weights_h2(const float* __restrict__ w, int K, int cin, int cout,
                                                       const float* __restrict__ col_scale, float mult,
                                                       unsigned short* __restrict__ wp, int trans = 0) {
    const long long total = (long long)K * cin * cout / 2;
    const int nch = cin / 32;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long r = i;
        const int k2 = (int)(r % 16); r /= 16;
        const int col = (int)(r % cout); r /= cout;
        const int c = (int)(r % nch); r /= nch;
        const int j = (int)r;
        // trans: w is [K][cout][cin] - the weights of the convolution whose transpose (input gradient) is being packed
        const float* p = trans ? w + ((long long)j * cout + col) * cin + c * 32 + 2 * k2
                               : w + ((long long)j * cin + c * 32 + 2 * k2) * cout + col;
        const float sc = (col_scale ? col_scale[col] : 1.f) * mult;
        unsigned h, l;
        split2h(p[0] * sc, p[trans ? 1 : cout] * sc, h, l);
        const long long base = ((long long)(j * nch + c) * 2 * cout + col) * 32 + 2 * k2;
        *reinterpret_cast<unsigned*>(wp + base) = h;
        *reinterpret_cast<unsigned*>(wp + base + (long long)cout * 32) = l;
    }
}

// wp6 layout (unsigned short): ((((j*nch + c)*3 + plane)*cout + col)*32 + k) for channel c*32 + k of offset j
// pack_weights_h2 for a whole network in ONE launch (cv_sp_pack_weights_h2_batch_f32): blockIdx.y = job
__global__ __launch_bounds__(256) void pack_weights_h2_batch(const cv_pack_job* __restrict__ jobs) {
    const cv_pack_job jb = jobs[blockIdx.y];
    const int K = jb.K, cin = jb.cin, cout = jb.cout, trans = jb.trans;
    const float* __restrict__ w = jb.w;
    unsigned short* __restrict__ wp = static_cast<unsigned short*>(jb.wp);
    const float mult = __uint_as_float((unsigned)(127 + jb.scale_log2) << 23);        // 2^scale_log2, |scale_log2| <= 60
    const long long total = (long long)K * cin * cout / 2;
    const int nch = cin / 32;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long r = i;
        const int k2 = (int)(r % 16); r /= 16;
        const int col = (int)(r % cout); r /= cout;
        const int c = (int)(r % nch); r /= nch;
        const int j = (int)r;
        const float* p = trans ? w + ((long long)j * cout + col) * cin + c * 32 + 2 * k2
                               : w + ((long long)j * cin + c * 32 + 2 * k2) * cout + col;
        unsigned h, l;
        split2h(p[0] * mult, p[trans ? 1 : cout] * mult, h, l);
        const long long base = ((long long)(j * nch + c) * 2 * cout + col) * 32 + 2 * k2;
        *reinterpret_cast<unsigned*>(wp + base) = h;
        *reinterpret_cast<unsigned*>(wp + base + (long long)cout * 32) = l;
    }
}

__global__ __launch_bounds__(256) void pack_weights_x6(const float* __restrict__ w, int K, int cin, int cout,
                                                       const float* __restrict__ col_scale,
                                                       unsigned short* __restrict__ wp, int trans = 0) {
    const long long total = (long long)K * cin * cout / 2;                   // pairs of consecutive k
    const int nch = cin / 32;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long r = i;
        const int k2 = (int)(r % 16); r /= 16;                               // k = 2*k2, 2*k2 + 1
        const int col = (int)(r % cout); r /= cout;
        const int c = (int)(r % nch); r /= nch;
        const int j = (int)r;
        const float* p = trans ? w + ((long long)j * cout + col) * cin + c * 32 + 2 * k2
                               : w + ((long long)j * cin + c * 32 + 2 * k2) * cout + col;
        unsigned h, m, l;
        const float sc = col_scale ? col_scale[col] : 1.f;
        split3(p[0] * sc, p[trans ? 1 : cout] * sc, h, m, l);
        const long long base = ((long long)(j * nch + c) * 3 * cout + col) * 32 + 2 * k2;
        *reinterpret_cast<unsigned*>(wp + base) = h;
        *reinterpret_cast<unsigned*>(wp + base + (long long)cout * 32) = m;
        *reinterpret_cast<unsigned*>(wp + base + 2ll * cout * 32) = l;
    }
}

// one bf16 plane (RNE): ((j*nch + c)*cout + col)*32 + k
__global__ __launch_bounds__(256) void pack_weights_b1(const float* __restrict__ w, int K, int cin, int cout,
                                                       const float* __restrict__ col_scale,
                                                       unsigned short* __restrict__ wp, int trans = 0) {
    const long long total = (long long)K * cin * cout / 2;
    const int nch = cin / 32;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long r = i;
        const int k2 = (int)(r % 16); r /= 16;
        const int col = (int)(r % cout); r /= cout;
        const int c = (int)(r % nch); r /= nch;
        const int j = (int)r;
        const float* p = trans ? w + ((long long)j * cout + col) * cin + c * 32 + 2 * k2
                               : w + ((long long)j * cin + c * 32 + 2 * k2) * cout + col;
        const float sc = col_scale ? col_scale[col] : 1.f;
        *reinterpret_cast<unsigned*>(wp + ((long long)(j * nch + c) * cout + col) * 32 + 2 * k2) =
            cvt_pk_bf16(p[0] * sc, p[trans ? 1 : cout] * sc);
    }
}

// weights of conv_stem_mfma: [K][cin][32] fp32 -> per (group of 16 offsets, input channel): two planes (h, l) of
// [col][half][8] fp16 = the B operand of v_mfma_f32_32x32x16_f16 with k = offset inside the group; offsets >= K are zero
__global__ __launch_bounds__(256) void pack_weights_stem_h2(const float* __restrict__ w, int K, int cin,
                                                            const float* __restrict__ col_scale, float mult,
                                                            unsigned short* __restrict__ wp) {
    const int total = 8 * cin * 32 * 2 * 4;           // (group, channel, col, half, pair of offsets)
    for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
        int r = t;
        const int q = r % 4; r /= 4;
        const int hf = r % 2; r /= 2;
        const int col = r % 32; r /= 32;
        const int ci = r % cin; r /= cin;
        const int g = r;
        const int j0 = g * 16 + hf * 8 + 2 * q;
        const float sc = (col_scale ? col_scale[col] : 1.f) * mult;
        const float v0 = j0 < K ? w[((long long)j0 * cin + ci) * 32 + col] * sc : 0.f;
        const float v1 = j0 + 1 < K ? w[((long long)(j0 + 1) * cin + ci) * 32 + col] * sc : 0.f;
        unsigned h, l;
        split2h(v0, v1, h, l);
        const long long base = ((((long long)(g * cin + ci) * 2) * 32 + col) * 2 + hf) * 8 + 2 * q;
        *reinterpret_cast<unsigned*>(wp + base) = h;
        *reinterpret_cast<unsigned*>(wp + base + 512) = l;
    }
}

// sort key of a row = bit mask of its valid neighbours among offsets [j_begin, j_end)
__global__ __launch_bounds__(256) void mask_keys(const int* __restrict__ nbr, long long n, int K, int j_begin,
                                                 int j_end, long long* __restrict__ keys) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= n) return;
    unsigned long long m = 0;
    for (int j = j_begin; j < j_end; ++j)
        if (nbr[i * K + j] >= 0) m |= 1ull << (j - j_begin);
    keys[i] = (long long)m;
}

// ---- row orders per offset group by counting sort on the group's neighbour bit mask (<= 10 bits).
// Three launches for all groups (blockIdx.y = group); LDS-aggregated histograms because global
// atomics on a few hundred hot counters serialise (~11 ns each on MI355X).
constexpr int MP_BINS = 1024;
constexpr int MP_THREADS = 1024;

__device__ __forceinline__ int group_mask(const int* __restrict__ nbr, long long row, long long n, int K, int jb, int je) {
    int m = 0;
    for (int j = jb; j < je; ++j)
        if (nbr[row * K + j] >= 0) m |= 1 << (j - jb);
    // sort key: rows with equal masks adjacent, and (when it fits the 1024 bins) ordered by the NUMBER of
    // offsets they need, so the tiles at the end of the order are the most expensive ones.
    // (Measured and dropped, profiles/README.md r2: masks sorted inside the eighths of the spatial row order with
    // tile t run on XCD t / (tiles / 8) - L2 hit rate of the ts1 conv 48 -> 63 %, memory-side fetch 192 -> 120 MB per
    // launch, and the launch 14 % SLOWER: the kernel is bound by its dependent round trips, not by fetch bandwidth,
    // and the cost ordering of the tiles is worth more than the hits.)
    if (je - jb <= 7) m |= __popc(m) << 7;
    (void)n;
    return m;
}

// the same key from the row's validity word (bit j = entry j >= 0, stored by the map builder: one load instead of je - jb)
__device__ __forceinline__ int group_mask_of_word(int word, int jb, int je) {
    int m = (int)(((unsigned)word >> jb) & ((1u << (je - jb)) - 1u));
    if (je - jb <= 7) m |= __popc(m) << 7;
    return m;
}

__global__ __launch_bounds__(MP_THREADS) void mp_hist(const int* __restrict__ nbr, long long n, int K, int groups,
                                                      int* __restrict__ hist /*[groups][MP_BINS]*/) {
    __shared__ int lh[MP_BINS];
    const int g = blockIdx.y;
    const int jb = K * g / groups, je = K * (g + 1) / groups;
    for (int i = threadIdx.x; i < MP_BINS; i += MP_THREADS) lh[i] = 0;
    __syncthreads();
    const long long row = blockIdx.x * (long long)MP_THREADS + threadIdx.x;
    if (row < n) atomicAdd(&lh[group_mask(nbr, row, n, K, jb, je)], 1);
    __syncthreads();
    for (int i = threadIdx.x; i < MP_BINS; i += MP_THREADS)
        if (lh[i]) atomicAdd(&hist[g * MP_BINS + i], lh[i]);
}

__global__ __launch_bounds__(MP_BINS) void mp_scan(int* __restrict__ hist) {   // exclusive, in place, per group
    __shared__ int s[MP_BINS];
    int* h = hist + blockIdx.x * MP_BINS;
    const int v = h[threadIdx.x];
    s[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < MP_BINS; off <<= 1) {
        const int t = threadIdx.x >= off ? s[threadIdx.x - off] : 0;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    h[threadIdx.x] = s[threadIdx.x] - v;
}

__global__ __launch_bounds__(MP_THREADS) void mp_scatter(const int* __restrict__ nbr, long long n, int K, int groups,
                                                         int* __restrict__ cursor, int* __restrict__ perm,
                                                         int* __restrict__ nbrp, int W) {
    // with the map rows (nbrp): behind them, one byte per (group, row) - does the row have a neighbour in the group at all?
    // (27 % of the rows of a scan have none below / above them: their partial sums are never written nor read, zskip)
    unsigned char* gv = nbrp ? reinterpret_cast<unsigned char*>(nbrp + (long long)groups * n * W) : nullptr;
    __shared__ int lh[MP_BINS];
    const int g = blockIdx.y;
    const int jb = K * g / groups, je = K * (g + 1) / groups;
    for (int i = threadIdx.x; i < MP_BINS; i += MP_THREADS) lh[i] = 0;
    __syncthreads();
    const long long row = blockIdx.x * (long long)MP_THREADS + threadIdx.x;
    int key = 0, rank = 0;
    if (row < n) {
        key = group_mask(nbr, row, n, K, jb, je);
        rank = atomicAdd(&lh[key], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MP_BINS; i += MP_THREADS)
        if (lh[i]) lh[i] = atomicAdd(&cursor[g * MP_BINS + i], lh[i]);
    __syncthreads();
    if (row < n) {
        const long long pos = (long long)g * n + lh[key] + rank;
        perm[pos] = (int)row;
        if (nbrp) {
            for (int j = jb; j < je; ++j) nbrp[pos * W + (j - jb)] = nbr[row * K + j];
            gv[(long long)g * n + row] = key != 0;
        }
    }
}

// the same three launches for several maps at once (every processing order of a scene): blockIdx.y = (job, group)
struct PermJobsDev {
    CvPermJob j[CV_MAX_PERM_JOBS];
    int group_begin[CV_MAX_PERM_JOBS + 1];
    int n;
};

__device__ __forceinline__ int perm_job_of(const PermJobsDev& jobs, int gy) {
    int ji = 0;
    while (ji + 1 < jobs.n && gy >= jobs.group_begin[ji + 1]) ++ji;
    return ji;
}

__global__ __launch_bounds__(MP_THREADS) void mp_hist_batch(const PermJobsDev jobs, int* __restrict__ hist) {
    __shared__ int lh[MP_BINS];
    const int ji = perm_job_of(jobs, blockIdx.y);
    const CvPermJob& jb = jobs.j[ji];
    const long long row = blockIdx.x * (long long)MP_THREADS + threadIdx.x;
    if (blockIdx.x * (long long)MP_THREADS >= jb.n) return;
    const int g = blockIdx.y - jobs.group_begin[ji];
    const int jlo = jb.K * g / jb.groups, jhi = jb.K * (g + 1) / jb.groups;
    for (int i = threadIdx.x; i < MP_BINS; i += MP_THREADS) lh[i] = 0;
    __syncthreads();
    if (row < jb.n)
        atomicAdd(&lh[jb.mask_words ? group_mask_of_word(jb.mask_words[row], jlo, jhi) : group_mask(jb.nbr, row, jb.n, jb.K, jlo, jhi)], 1);
    __syncthreads();
    for (int i = threadIdx.x; i < MP_BINS; i += MP_THREADS)
        if (lh[i]) atomicAdd(&hist[blockIdx.y * MP_BINS + i], lh[i]);
}

// (round 5: no scan launch between the histogram and the scatter of the batched orders - a scatter workgroup scans its group's
// 1024 bin counts itself (one per thread) and claims its rows' places from a SECOND zeroed array of running counts per bin)
__global__ __launch_bounds__(MP_THREADS) void mp_scatter_batch(const PermJobsDev jobs, const int* __restrict__ hist,
                                                               int* __restrict__ cursor) {
    static_assert(MP_THREADS == MP_BINS, "one bin per thread in the scan");
    __shared__ int lh[MP_BINS];
    __shared__ int pre[MP_BINS];
    __shared__ int wtot[MP_THREADS / 64];
    const int ji = perm_job_of(jobs, blockIdx.y);
    const CvPermJob& jb = jobs.j[ji];
    if (blockIdx.x * (long long)MP_THREADS >= jb.n) return;
    const int g = blockIdx.y - jobs.group_begin[ji];
    const int K = jb.K, jlo = K * g / jb.groups, jhi = K * (g + 1) / jb.groups, W = (K + jb.groups - 1) / jb.groups;
    int* nbrp = jb.with_map ? jb.perm + (long long)jb.groups * jb.n : nullptr;
    for (int i = threadIdx.x; i < MP_BINS; i += MP_THREADS) lh[i] = 0;
    {   // exclusive scan of the group's bin counts: first slot of every bin
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int v = hist[blockIdx.y * MP_BINS + threadIdx.x];
        int incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int base = 0;
#pragma unroll
        for (int w = 0; w < MP_THREADS / 64; ++w) base += w < wave ? wtot[w] : 0;
        pre[threadIdx.x] = base + incl - v;
    }
    __syncthreads();
    const long long row = blockIdx.x * (long long)MP_THREADS + threadIdx.x;
    int key = 0, rank = 0;
    if (row < jb.n) {
        key = jb.mask_words ? group_mask_of_word(jb.mask_words[row], jlo, jhi) : group_mask(jb.nbr, row, jb.n, K, jlo, jhi);
        rank = atomicAdd(&lh[key], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < MP_BINS; i += MP_THREADS)
        if (lh[i]) lh[i] = pre[i] + atomicAdd(&cursor[blockIdx.y * MP_BINS + i], lh[i]);
    __syncthreads();
    long long pos = 0;
    if (row < jb.n) {
        pos = (long long)g * jb.n + lh[key] + rank;
        jb.perm[pos] = (int)row;
        if (nbrp) reinterpret_cast<unsigned char*>(nbrp + (long long)jb.groups * jb.n * W)[(long long)g * jb.n + row] = key != 0;
    }
    if (!nbrp) return;
    // the map rows in processing order, copied by the whole workgroup: adjacent lanes read and write a row's adjacent entries
    // (a thread copying its own row issued jhi - jlo scattered 4-byte stores one after the other).  Places of the workgroup's
    // rows through LDS (`pre` is free: its last readers are in front of the barrier above), 32 bits: pos - g * n < n < 2^31
    pre[threadIdx.x] = (int)(pos - (long long)g * jb.n);
    __syncthreads();
    const long long row0 = blockIdx.x * (long long)MP_THREADS;
    const int nrow = (int)((jb.n - row0 < MP_THREADS) ? jb.n - row0 : MP_THREADS), Wg = jhi - jlo;
    const int total = nrow * Wg;
    const int* src0 = jb.nbr + row0 * K + jlo;
    int* dst0 = nbrp + (long long)g * jb.n * W;
    for (int e0 = threadIdx.x; e0 < total; e0 += 3 * MP_THREADS) {       // three entries in flight per thread
        int v[3], r[3], jj[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int e = e0 + q * MP_THREADS;
            r[q] = Wg == 9 ? (int)((unsigned)e / 9u) : (int)((unsigned)e / (unsigned)Wg);
            jj[q] = e - r[q] * Wg;
            v[q] = e < total ? src0[(long long)r[q] * K + jj[q]] : 0;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (e0 + q * MP_THREADS < total) dst0[(long long)pre[r[q]] * W + jj[q]] = v[q];
    }
}

}  // namespace

int cv_sp_mask_perms_batch(const CvPermJob* jobs, int n_jobs, void* d_ws, size_t ws_bytes, void* stream, bool pre_zeroed) {
    CV_REQUIRE(jobs && d_ws && n_jobs > 0 && n_jobs <= CV_MAX_PERM_JOBS, CV_EINVAL, "bad mask perm batch");
    PermJobsDev d;
    d.n = n_jobs;
    int groups = 0;
    long long max_n = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const CvPermJob& j = jobs[i];
        CV_REQUIRE(j.nbr && j.perm && j.n > 0 && j.K > 0 && j.groups >= 1 && j.groups <= j.K, CV_EINVAL,
                   "bad mask perm job %d", i);
        CV_REQUIRE((j.K + j.groups - 1) / j.groups <= 10, CV_EINVAL, "at most 10 kernel offsets per group");
        CV_REQUIRE(!j.mask_words || j.K <= 32, CV_EINVAL, "validity words hold at most 32 kernel offsets");
        d.j[i] = j;
        d.group_begin[i] = groups;
        groups += j.groups;
        max_n = std::max(max_n, j.n);
    }
    d.group_begin[n_jobs] = groups;
    // workspace: [groups][1024] bin counts, then [groups][1024] running counts of the scatter (both zero at the start)
    CV_REQUIRE(ws_bytes >= sizeof(int) * (size_t)groups * MP_BINS * 2, CV_ENOMEM, "workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* hist = static_cast<int*>(d_ws);
    int* cursor = hist + (size_t)groups * MP_BINS;
    if (!pre_zeroed) CV_HIP_CHECK(hipMemsetAsync(hist, 0, sizeof(int) * (size_t)groups * MP_BINS * 2, st));
    dim3 grid((unsigned)((max_n + MP_THREADS - 1) / MP_THREADS), (unsigned)groups);
    mp_hist_batch<<<grid, MP_THREADS, 0, st>>>(d, hist);
    CV_LAUNCH_CHECK();
    mp_scatter_batch<<<grid, MP_THREADS, 0, st>>>(d, hist, cursor);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

extern "C" {

// d_keys[n] = bit mask of valid neighbours among kernel offsets [j_begin, j_end) of each output row.
// Sorting rows by this key groups rows that need the same offsets (cv_conv_desc.row_perm).
int cv_sp_mask_keys(const int32_t* d_nbr, long long n, int K, int j_begin, int j_end, long long* d_keys,
                    void* stream) {
    CV_REQUIRE(d_nbr && d_keys && n > 0 && K > 0 && j_begin >= 0 && j_begin < j_end && j_end <= K &&
                   j_end - j_begin <= 63, CV_EINVAL, "bad mask key arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    mask_keys<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(d_nbr, n, K, j_begin, j_end, d_keys);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

// d_perm[groups][n] = rows ordered by the neighbour bit mask of each contiguous group of the K offsets
// (ceil(K/groups) <= 10).  d_ws: groups*1024 ints of scratch.  Asynchronous, three launches.
int cv_sp_mask_perms(const int32_t* d_nbr, long long n, int K, int groups, int32_t* d_perm, void* d_ws,
                     size_t ws_bytes, int with_map, void* stream) {
    CV_REQUIRE(d_nbr && d_perm && d_ws && n > 0 && K > 0 && groups >= 1 && groups <= K, CV_EINVAL,
               "bad mask perm arguments");
    CV_REQUIRE((K + groups - 1) / groups <= 10, CV_EINVAL, "at most 10 kernel offsets per group");
    CV_REQUIRE(ws_bytes >= sizeof(int) * (size_t)groups * MP_BINS, CV_ENOMEM, "workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* hist = static_cast<int*>(d_ws);
    CV_HIP_CHECK(hipMemsetAsync(hist, 0, sizeof(int) * (size_t)groups * MP_BINS, st));
    dim3 grid((unsigned)((n + MP_THREADS - 1) / MP_THREADS), (unsigned)groups);
    mp_hist<<<grid, MP_THREADS, 0, st>>>(d_nbr, n, K, groups, hist);
    CV_LAUNCH_CHECK();
    mp_scan<<<groups, MP_BINS, 0, st>>>(hist);
    CV_LAUNCH_CHECK();
    mp_scatter<<<grid, MP_THREADS, 0, st>>>(d_nbr, n, K, groups, hist, d_perm,
                                            with_map ? d_perm + (long long)groups * n : nullptr, (K + groups - 1) / groups);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

// What the four weight-packer entry points below share: their argument checks, in their order, and the grid of the launch.
// name / wp: the packer and its output argument as the messages spell them; cin_fmt: the entry point's wording for Cin (takes
// name and Cin); own_failure: the message of the check that only this entry point makes, when it failed, else NULL.
constexpr const char* PACK_CIN = "%s needs Cin %% 32 == 0 (got %d)";
static int pack_entry(const char* name, const char* wp, const float* d_w, const void* d_wp, int K, int cin, int cout,
                      const char* cin_fmt, const char* own_failure, unsigned* grid) {
    CV_REQUIRE(d_w && d_wp && K > 0 && cin > 0 && cout > 0, CV_EINVAL, "bad %s arguments", name);
    CV_REQUIRE(cin % 32 == 0, CV_EINVAL, cin_fmt, name, cin);
    CV_REQUIRE(!own_failure, CV_EINVAL, "%s", own_failure);
    CV_REQUIRE(aligned16(d_wp), CV_EINVAL, "%s must be 16-byte aligned", wp);
    const long long total = (long long)K * cin * cout / 2;
    *grid = (unsigned)std::min<long long>((total + 255) / 256, 8192);
    return CV_OK;
}

// d_wp6[3*K*cin*cout] (16-bit words) = d_w[K][cin][cout] split into three bf16 pieces per value and laid out per
// (offset, 32-channel chunk) as [piece][cout][32 channels] for conv_rows_wp (cin % 32 == 0).  Redo when weights change.
int cv_sp_pack_weights_x6_f32(const float* d_w, int K, int cin, int cout, const float* d_col_scale, void* d_wp6,
                              void* stream) {
    unsigned grid;
    if (const int e = pack_entry("pack_weights_x6", "d_wp6", d_w, d_wp6, K, cin, cout, PACK_CIN, nullptr, &grid)) return e;
    pack_weights_x6<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(d_w, K, cin, cout, d_col_scale,
                                                                        static_cast<unsigned short*>(d_wp6));
    CV_LAUNCH_CHECK();
    return CV_OK;
}

// d_wp[K*cin*cout] (16-bit words) = d_w * d_col_scale rounded to bf16 (RNE), laid out per (offset, 32-channel
// chunk) as [cout][32 channels] (cv_conv_desc.weight_pieces = 1: the opt-in bf16 compute mode).
int cv_sp_pack_weights_bf16_f32(const float* d_w, int K, int cin, int cout, const float* d_col_scale, void* d_wp,
                                void* stream) {
    unsigned grid;
    if (const int e = pack_entry("pack_weights_bf16", "d_wp", d_w, d_wp, K, cin, cout, PACK_CIN, nullptr, &grid)) return e;
    pack_weights_b1<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(d_w, K, cin, cout, d_col_scale,
                                                                        static_cast<unsigned short*>(d_wp));
    CV_LAUNCH_CHECK();
    return CV_OK;
}

// d_wp[2*K*cin*cout] (16-bit words) = d_w * d_col_scale * 2^scale_log2 split into two fp16 pieces per value, laid
// out per (offset, 32-channel chunk) as [piece][cout][32 channels] (cv_conv_desc.weight_pieces = 2; pass
// acc_scale = 2^-scale_log2).  Choose scale_log2 so that the largest scaled magnitude is about 2^13: the low pieces
// of weights down to 2^-14 of the largest one then stay normal fp16 numbers.
int cv_sp_pack_weights_h2_f32(const float* d_w, int K, int cin, int cout, const float* d_col_scale, int scale_log2,
                              void* d_wp, void* stream) {
    unsigned grid;
    const char* bad_scale = scale_log2 >= -60 && scale_log2 <= 60 ? nullptr : "scale_log2 out of range";
    if (const int e = pack_entry("pack_weights_h2", "d_wp", d_w, d_wp, K, cin, cout, PACK_CIN, bad_scale, &grid)) return e;
    pack_weights_h2<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(d_w, K, cin, cout, d_col_scale, ldexpf(1.f, scale_log2),
                                                                        static_cast<unsigned short*>(d_wp));
    CV_LAUNCH_CHECK();
    return CV_OK;
}

// Packed weights of the TRANSPOSED convolution (the input gradient: dX = conv over the transposed map with W_j^T) straight
// from the forward weights d_w[K][rows][cols]: the packed tensor is that of W'[K][cin = cols][cout = rows] with
// W'[j][a][b] = d_w[j][b][a] - no transposed copy of the weights per layer and step.  pieces 3: bf16 triples, 2: fp16 pairs
// (times 2^scale_log2), 1: one bf16 plane.
int cv_sp_pack_weights_t_f32(const float* d_w, int K, int rows, int cols, int pieces, int scale_log2, void* d_wp, void* stream) {
    const int cin = cols, cout = rows;
    unsigned grid;
    const char* bad_pieces = pieces >= 1 && pieces <= 3 && scale_log2 >= -60 && scale_log2 <= 60 ? nullptr : "pieces is 1, 2 or 3";
    if (const int e = pack_entry("pack_weights_t", "d_wp", d_w, d_wp, K, cin, cout,
                                 "%s needs %d (the input channels of the transposed convolution) %% 32 == 0", bad_pieces, &grid))
        return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned short* wp = static_cast<unsigned short*>(d_wp);
    if (pieces == 3) pack_weights_x6<<<grid, 256, 0, st>>>(d_w, K, cin, cout, nullptr, wp, 1);
    else if (pieces == 2) pack_weights_h2<<<grid, 256, 0, st>>>(d_w, K, cin, cout, nullptr, ldexpf(1.f, scale_log2), wp, 1);
    else pack_weights_b1<<<grid, 256, 0, st>>>(d_w, K, cin, cout, nullptr, wp, 1);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_sp_pack_weights_h2_batch_f32(const cv_pack_job* h_jobs, int n_jobs, void* d_jobs, void* stream) {
    CV_REQUIRE(n_jobs >= 0 && (n_jobs == 0 || (h_jobs && d_jobs)), CV_EINVAL, "bad pack batch");
    if (n_jobs == 0) return CV_OK;
    for (int i = 0; i < n_jobs; ++i) {
        const cv_pack_job& j = h_jobs[i];
        CV_REQUIRE(j.w && j.wp && j.K > 0 && j.cin > 0 && j.cout > 0 && j.cin % 32 == 0, CV_EINVAL,
                   "pack job %d: null pointer or Cin %% 32 != 0 (K %d, Cin %d, Cout %d)", i, j.K, j.cin, j.cout);
        CV_REQUIRE(j.scale_log2 >= -60 && j.scale_log2 <= 60 && (j.trans == 0 || j.trans == 1), CV_EINVAL, "pack job %d: scale_log2 / trans out of range", i);
        CV_REQUIRE((reinterpret_cast<uintptr_t>(j.wp) & 15) == 0, CV_EINVAL, "pack job %d: wp must be 16-byte aligned", i);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    CV_HIP_CHECK(hipMemcpyAsync(d_jobs, h_jobs, sizeof(cv_pack_job) * (size_t)n_jobs, hipMemcpyHostToDevice, st));
    pack_weights_h2_batch<<<dim3(64, (unsigned)n_jobs), 256, 0, st>>>(static_cast<const cv_pack_job*>(d_jobs));
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_sp_pack_weights_stem_h2_f32(const float* d_w, int K, int cin, const float* d_col_scale, int scale_log2, void* d_wp,
                                   void* stream) {
    CV_REQUIRE(d_w && d_wp && K > 0 && K <= 128 && (cin == 3 || cin == 6), CV_EINVAL,
               "stem weights: K <= 128, Cin 3 or 6, 32 output channels");
    CV_REQUIRE(scale_log2 >= -100 && scale_log2 <= 100, CV_EINVAL, "bad scale exponent");
    pack_weights_stem_h2<<<64, 256, 0, static_cast<hipStream_t>(stream)>>>(d_w, K, cin, d_col_scale, ldexpf(1.f, scale_log2),
                                                                           static_cast<unsigned short*>(d_wp));
    CV_LAUNCH_CHECK();
    return CV_OK;
}

}  // extern "C"
