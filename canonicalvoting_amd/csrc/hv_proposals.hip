// SUN RGB-D proposal sampler on the device (sunrgbd/brnetcanon.py:123-159, the part of HoughVotingModule.forward behind the
// vote): cv_prop_columns_f32, cv_prop_select_f32 and the per-cloud front's cv_prop_cloud_ranges_i32.  Contract: cv_hip.h.
//
// Columns, two launches.
//   prop_columns  one lane per (x, z) column of grid_obj [X][Y][Z]: the grid is Z-fastest, so adjacent lanes read adjacent
//                 z for every y.  Maximum over y with the FIRST y that attains it, NaN as the maximum (first NaN wins);
//                 dist = (m + 1e-7f)^pow.
//   prop_finish   ONE workgroup.  Lane t owns the contiguous cells [t * L, (t + 1) * L), L = ceil(n / 256): it adds them in
//                 cell order in fp64 (T_t) and notes a non-finite one; lane 0 walks the 256 totals in lane order (O_0 = 0,
//                 O_{t+1} = O_t + T_t), which gives the sum and the uniform decision; then every lane writes either 1.0f and
//                 the exact prefix c + 1, or cdf[c] = O_t + (its running local sum).  Non-decreasing by construction: inside
//                 a lane the local sum grows and x -> O_t + x is monotone after rounding; the last entry of lane t is
//                 O_t + T_t = O_{t+1}, which the first entry of lane t + 1 cannot fall below.  (A tree scan over the lanes
//                 would not guarantee that: neighbouring entries would be rounded along different trees.)
// Select, one launch of ONE workgroup (SEL_THREADS lanes): per round, pass A walks the round's draws in chunks of one draw
// per lane - cell, world point, nearest seed with the seeds staged through LDS in tiles of SEED_TILE - and leaves
// cell * 2 + near in the workspace; pass B walks the same chunks in order and compacts the kept draws behind the rows that
// exist (ballot + popcount inside a wave, the 16 wave counts in LDS), so rows keep draw order.
//
// No atomics; every order depends on the sizes alone, so all outputs are the same bytes on every run and stream.  Built with
// -ffp-contract=off (csrc/build.py STRICT): the expressions are evaluated as written.
#include "cv_common.h"

#include <climits>
#include <cmath>

namespace {

constexpr int COL_THREADS = 256;
constexpr int FIN_THREADS = 256;
constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int SEED_TILE = 1024;                   // seeds per LDS tile (12 KB)
constexpr int RNG_THREADS = 256;

__global__ __launch_bounds__(COL_THREADS) void prop_columns(const float* __restrict__ grid, int X, int Y, int Z, double pw,
                                                            int use_sqrt, float* __restrict__ dist, int32_t* __restrict__ yidx) {
    const long long c = blockIdx.x * (long long)COL_THREADS + threadIdx.x;
    if (c >= (long long)X * Z) return;
    const int x = (int)(c / Z), z = (int)(c % Z);
    const float* col = grid + (long long)x * Y * Z + z;
    float m = col[0];
    int iy = 0;
    for (int y = 1; y < Y; ++y) {
        const float v = col[(long long)y * Z];
        // a strictly larger value, or the first NaN (torch.max / argmax: NaN is the maximum)
        if (v > m || (v != v && m == m)) {
            m = v;
            iy = y;
        }
    }
    const float b = m + 1e-7f;
    dist[c] = use_sqrt ? sqrtf(b) : (float)pow((double)b, pw);
    yidx[c] = iy;
}

__global__ __launch_bounds__(FIN_THREADS) void prop_finish(float* __restrict__ dist, long long n, double* __restrict__ cdf,
                                                           int32_t* __restrict__ flags) {
    __shared__ double tot[FIN_THREADS];
    __shared__ double off[FIN_THREADS];
    __shared__ int bad[FIN_THREADS];
    __shared__ int s_uniform;
    const int t = threadIdx.x;
    const long long L = (n + FIN_THREADS - 1) / FIN_THREADS;
    const long long b = min(n, t * L), e = min(n, b + L);
    double sum = 0.0;
    int nonfinite = 0;
    for (long long i = b; i < e; ++i) {
        const float v = dist[i];
        nonfinite |= !(fabsf(v) <= 3.402823466e38f);        // NaN or an infinity
        sum += (double)v;
    }
    tot[t] = sum;
    bad[t] = nonfinite;
    __syncthreads();
    if (t == 0) {
        double run = 0.0;
        int any = 0;
        for (int k = 0; k < FIN_THREADS; ++k) {
            off[k] = run;
            run += tot[k];
            any |= bad[k];
        }
        const int uniform = any || run < (double)1e-7f;      // brnetcanon.py:128
        flags[0] = uniform;
        flags[1] = any;
        s_uniform = uniform;
    }
    __syncthreads();
    if (s_uniform) {
        for (long long i = b; i < e; ++i) {
            dist[i] = 1.0f;
            cdf[i] = (double)(i + 1);
        }
    } else {
        const double o = off[t];
        double local = 0.0;
        for (long long i = b; i < e; ++i) {
            local += (double)dist[i];
            cdf[i] = o + local;
        }
    }
}

__global__ __launch_bounds__(SEL_THREADS) void prop_select(const cv_prop_select_desc d, int32_t* __restrict__ code) {
    __shared__ float seeds[SEED_TILE * 3];
    __shared__ int wave_cnt[SEL_WAVES];
    __shared__ int s_any;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int Y = d.dims[1], Z = d.dims[2];
    const int n = d.dims[0] * Z;
    const int S = d.per_round, P = d.num_proposal, V = d.n_seeds;
    const double total = d.d_uniform ? d.d_cdf[n - 1] : 0.0;
    int filled = d.start, used = 0;
    for (int r = 0; r < d.rounds && filled < P; ++r) {
        ++used;
        if (t == 0) s_any = 0;
        // ---- pass A: cell and near flag of every draw of the round
        int any_mine = 0;
        for (int base = 0; base < S; base += SEL_THREADS) {
            const int i = base + t;
            const bool live = i < S;
            int cell = 0;
            float wx = 0.0f, wy = 0.0f, wz = 0.0f;
            if (live) {
                const long long at = (long long)r * S + i;
                if (d.d_draws) {
                    const long long s = d.d_draws[at];
                    cell = (int)(s < 0 ? 0 : (s >= n ? n - 1 : s));
                } else {
                    const double tt = (double)d.d_uniform[at] * total;
                    int lo = 0, hi = n - 1;                 // the first cell whose cdf exceeds tt, the last when none does
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (d.d_cdf[mid] > tt) hi = mid; else lo = mid + 1;
                    }
                    cell = lo;
                }
                const int ix = cell / Z, iz = cell % Z;
                const int iy = min(max(d.d_yidx[cell], 0), Y - 1);
                wx = ((float)ix * d.res) + d.corner[0];
                wy = ((float)iy * d.res) + d.corner[1];
                wz = ((float)iz * d.res) + d.corner[2];
            }
            float best = INFINITY;
            for (int v0 = 0; v0 < V; v0 += SEED_TILE) {
                const int cnt = min(SEED_TILE, V - v0);
                __syncthreads();                            // the tile before has been read by everyone
                for (int k = t; k < cnt * 3; k += SEL_THREADS) seeds[k] = d.d_seeds[(long long)v0 * 3 + k];
                __syncthreads();
                if (live) {
                    for (int k = 0; k < cnt; ++k) {
                        const float dx = wx - seeds[3 * k], dy = wy - seeds[3 * k + 1], dz = wz - seeds[3 * k + 2];
                        const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
                        best = (d2 < best || d2 != d2) ? d2 : best;     // a NaN wins and stays (torch.min)
                    }
                }
            }
            if (live) {
                const int near = sqrtf(best) < d.radius;
                code[i] = (cell << 1) | near;               // read back by this same lane in pass B
                any_mine |= near;
            }
        }
        __syncthreads();                                    // s_any = 0 has landed
        if (any_mine) s_any = 1;
        __syncthreads();
        const int any = s_any;
        // ---- pass B: ordered compaction of the kept draws behind the rows that exist
        for (int base = 0; base < S && filled < P; base += SEL_THREADS) {
            const int i = base + t;
            const int c = i < S ? code[i] : 0;
            const bool keep = i < S && (!any || (c & 1));
            const unsigned long long votes = __ballot(keep);
            if (lane == 0) wave_cnt[wave] = __popcll(votes);
            __syncthreads();
            int before = 0, kept = 0;
            for (int w = 0; w < SEL_WAVES; ++w) {
                const int k = wave_cnt[w];
                before += w < wave ? k : 0;
                kept += k;
            }
            const long long row = (long long)filled + before + __popcll(votes & ((1ull << lane) - 1ull));
            if (keep && row < P) {
                const int cell = c >> 1;
                const int ix = cell / Z, iz = cell % Z;
                const int iy = min(max(d.d_yidx[cell], 0), Y - 1);
                d.d_cand[row * 3 + 0] = ((float)ix * d.res) + d.corner[0];
                d.d_cand[row * 3 + 1] = ((float)iy * d.res) + d.corner[1];
                d.d_cand[row * 3 + 2] = ((float)iz * d.res) + d.corner[2];
                const float* sc = d.d_grid_scale + (((long long)ix * Y + iy) * Z + iz) * 3;
                d.d_scale[row * 3 + 0] = sc[0];
                d.d_scale[row * 3 + 1] = sc[1];
                d.d_scale[row * 3 + 2] = sc[2];
            }
            filled = (int)min((long long)P, (long long)filled + kept);
            __syncthreads();                                // wave_cnt is rewritten by the next chunk
        }
    }
    if (t == 0) {
        d.d_info[0] = filled;
        d.d_info[1] = used;
    }
}

// workgroup b: rows of cloud b by two bisections of the batch column, then min / max of its coordinates
__global__ __launch_bounds__(RNG_THREADS) void prop_cloud_ranges(const int32_t* __restrict__ coords4, long long n,
                                                                 int32_t* __restrict__ out) {
    __shared__ int lo3[RNG_THREADS][3];
    __shared__ int hi3[RNG_THREADS][3];
    const int b = blockIdx.x, t = threadIdx.x;
    long long first[2];
    for (int k = 0; k < 2; ++k) {                           // the first row whose batch index is >= b + k
        long long lo = 0, hi = n;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (coords4[mid * 4] >= b + k) hi = mid; else lo = mid + 1;
        }
        first[k] = lo;
    }
    int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
    for (long long i = first[0] + t; i < first[1]; i += RNG_THREADS)
        for (int c = 0; c < 3; ++c) {
            const int v = coords4[i * 4 + 1 + c];
            mn[c] = min(mn[c], v);
            mx[c] = max(mx[c], v);
        }
    for (int c = 0; c < 3; ++c) {
        lo3[t][c] = mn[c];
        hi3[t][c] = mx[c];
    }
    __syncthreads();
    for (int half = RNG_THREADS / 2; half > 0; half >>= 1) {
        if (t < half)
            for (int c = 0; c < 3; ++c) {
                lo3[t][c] = min(lo3[t][c], lo3[t + half][c]);
                hi3[t][c] = max(hi3[t][c], hi3[t + half][c]);
            }
        __syncthreads();
    }
    if (t == 0) {
        int32_t* o = out + (long long)b * 8;
        o[0] = (int32_t)first[0];
        o[1] = (int32_t)first[1];
        for (int c = 0; c < 3; ++c) {
            o[2 + c] = lo3[0][c];
            o[5 + c] = hi3[0][c];
        }
    }
}

int check_dims(const int* dims) {
    CV_REQUIRE(dims, CV_EINVAL, "null pointer argument (dims)");
    CV_REQUIRE(dims[0] > 0 && dims[1] > 0 && dims[2] > 0, CV_EINVAL, "grid dims %d x %d x %d: all must be positive", dims[0],
               dims[1], dims[2]);
    CV_REQUIRE((long long)dims[0] * dims[2] <= (1ll << 30) && (long long)dims[0] * dims[1] * dims[2] < (1ll << 31), CV_EINVAL,
               "grid dims %d x %d x %d beyond the sampler's index range", dims[0], dims[1], dims[2]);
    return CV_OK;
}

}  // namespace

extern "C" {

size_t cv_sizeof_prop_select_desc(void) { return sizeof(cv_prop_select_desc); }

size_t cv_prop_workspace_bytes(int per_round) {
    return per_round < 1 ? 0 : cv_align_up((size_t)per_round * sizeof(int32_t), 256);
}

int cv_prop_columns_f32(const float* d_grid_obj, const int* dims, double pw, float* d_dist, int32_t* d_yidx, double* d_cdf,
                        int32_t* d_flags, void* stream) {
    CV_REQUIRE(d_grid_obj && d_dist && d_yidx && d_cdf && d_flags, CV_EINVAL, "null pointer argument");
    if (int rc = check_dims(dims)) return rc;
    CV_REQUIRE(pw == pw, CV_EINVAL, "pow is NaN");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long n = (long long)dims[0] * dims[2];
    prop_columns<<<(unsigned)((n + COL_THREADS - 1) / COL_THREADS), COL_THREADS, 0, st>>>(d_grid_obj, dims[0], dims[1], dims[2],
                                                                                          pw, pw == 0.5, d_dist, d_yidx);
    CV_LAUNCH_CHECK();
    prop_finish<<<1, FIN_THREADS, 0, st>>>(d_dist, n, d_cdf, d_flags);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

int cv_prop_select_f32(const cv_prop_select_desc* desc, void* stream) {
    CV_REQUIRE(desc, CV_EINVAL, "null proposal-select descriptor");
    const cv_prop_select_desc& d = *desc;
    CV_REQUIRE(d.d_grid_scale && d.d_yidx && d.d_seeds && d.d_cand && d.d_scale && d.d_info, CV_EINVAL, "null pointer argument");
    if (int rc = check_dims(d.dims)) return rc;
    CV_REQUIRE((d.d_draws != nullptr) != (d.d_uniform != nullptr), CV_EINVAL,
               "exactly one of d_draws / d_uniform must be given (got %s)", d.d_draws ? "both" : "neither");
    CV_REQUIRE(d.d_draws || d.d_cdf, CV_EINVAL, "null pointer argument (d_cdf, read in uniform mode)");
    CV_REQUIRE(d.rounds >= 1 && d.per_round >= 1, CV_EINVAL, "rounds %d / per_round %d: both must be at least 1", d.rounds,
               d.per_round);
    CV_REQUIRE(d.num_proposal >= 1 && d.start >= 0 && d.start <= d.num_proposal, CV_EINVAL,
               "start %d outside 0 .. num_proposal %d", d.start, d.num_proposal);
    CV_REQUIRE(d.n_seeds >= 1, CV_EINVAL, "%d seeds: the nearest of none is undefined", d.n_seeds);
    CV_REQUIRE(d.res == d.res && d.radius == d.radius, CV_EINVAL, "res / radius is NaN");
    const size_t need = cv_prop_workspace_bytes(d.per_round);
    CV_REQUIRE(d.d_ws && d.ws_bytes >= need, CV_ENOMEM, "proposal-select workspace too small (needs %zu bytes)", need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    prop_select<<<1, SEL_THREADS, 0, st>>>(d, static_cast<int32_t*>(d.d_ws));
    CV_LAUNCH_CHECK();
    if (d.h_info) CV_HIP_CHECK(hipMemcpyAsync(d.h_info, d.d_info, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    return CV_OK;
}

int cv_prop_cloud_ranges_i32(const int32_t* d_coords4, long long n, int n_clouds, int32_t* d_out, int32_t* h_out, void* stream) {
    CV_REQUIRE(d_coords4 && d_out, CV_EINVAL, "null pointer argument");
    CV_REQUIRE(n >= 1 && n < (1ll << 31) && n_clouds >= 1 && n_clouds <= 65536, CV_EINVAL, "%lld rows / %d clouds out of range", n,
               n_clouds);
    hipStream_t st = static_cast<hipStream_t>(stream);
    prop_cloud_ranges<<<(unsigned)n_clouds, RNG_THREADS, 0, st>>>(d_coords4, n, d_out);
    CV_LAUNCH_CHECK();
    if (h_out) CV_HIP_CHECK(hipMemcpyAsync(h_out, d_out, (size_t)n_clouds * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    return CV_OK;
}

}  // extern "C"
