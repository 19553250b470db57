// Training batch from raw scans (cv_sp_scan_rows_f32): the features and the three label arrays of the kept rows of a
// voxelised batch, computed per row from the raw per-vertex arrays - what ScanNetXYZProbMultiDataset.__getitem__
// (utils/dataloader.py:118-210) computes for EVERY vertex on the host and then gathers by the first-point index.
//
// One launch behind the voxeliser, laid out like voxel_rows (sparse_coords.hip, section 7): every output owns a range of
// workgroups that strides over its n * width elements, so adjacent lanes write adjacent destination words.  The model table
// ([n_models] x (12 fp64 + 3 fp32 + 1 int32)) and the colour table ([n_clouds][6] fp64) are a few hundred bytes and stay in
// cache; the per-vertex reads follow `index`, which ascends.  About 100 B per row: the launch is bound by its latency.
//
// Built with -ffp-contract=off (csrc/build.py STRICT): the label transform is the fp64 expression of cv_hip.h as written,
// and the colour steps round to fp32 one at a time, the way numpy's in-place `float32 op= float64` does.
#include "cv_common.h"

#include <algorithm>

namespace {

constexpr int SCAN_ROWS_MAX_BLOCKS = 512;          // per output: 131072 threads, then the loops stride
constexpr long long BACKGROUND_CLASS = 9;          // utils/dataloader.py:166

struct ScanRowsDev {
    cv_scan_rows_desc d;
    int fw;                                         // feature width: 3, or 6 with use_xyz
    int block_begin[5];                             // feats, xyz, scale, cls: output s owns [s], [s + 1])
};

int blocks_for(long long elems) { return (int)std::min<long long>((elems + 255) / 256, SCAN_ROWS_MAX_BLOCKS); }

// the model of a raw vertex: a row of the model table, or -1 (background; also what an owner outside the table reads as)
__device__ __forceinline__ int model_of(const cv_scan_rows_desc& d, int v) {
    const int o = d.d_owner[v];
    return (unsigned)o < (unsigned)d.n_models ? o : -1;
}

__global__ __launch_bounds__(256) void scan_rows(const ScanRowsDev a) {
    const cv_scan_rows_desc& d = a.d;
    int s = 0;
    while (s < 3 && (int)blockIdx.x >= a.block_begin[s + 1]) ++s;
    const int nblk = a.block_begin[s + 1] - a.block_begin[s], blk = blockIdx.x - a.block_begin[s];
    const long long first = blk * 256ll + threadIdx.x, step = (long long)nblk * 256;
    if (s == 0) {
        const int fw = a.fw, c0 = fw - 3;           // colour columns: [c0, fw)
        for (long long e = first; e < d.n * fw; e += step) {
            const long long i = e / fw;
            const int c = (int)(e - i * fw);
            const long long v = d.d_index[i];
            float x;
            if (c < c0) {
                x = d.d_points[v * d.points_ld + c];
            } else {
                const int k = c - c0;
                x = (float)((double)d.d_rgb[v * 3 + k] / 255.0);
                if (d.d_colour) {
                    const int b = d.d_coords4[4 * i];
                    const double* t = d.d_colour + 6ll * ((unsigned)b < (unsigned)d.n_clouds ? b : 0);
                    x = (float)((double)x * t[k]);
                    x = (float)((double)x + t[3 + k]);
                    x = (float)((double)x + d.d_jitter[v]);
                    x = fminf(fmaxf(x, 0.0f), 1.0f);
                }
                if (d.recentre) x = x * 2.0f - 1.0f;
            }
            d.d_feats[i * d.feats_ld + c] = x;
        }
    } else if (s == 1) {
        for (long long e = first; e < d.n * 3; e += step) {
            const long long i = e / 3;
            const int r = (int)(e - i * 3);
            const long long v = d.d_index[i];
            const int o = model_of(d, (int)v);
            float x = 0.0f;
            if (o >= 0) {
                const double* m = d.d_minv + 12ll * o + 4 * r;
                const float* p = d.d_points + v * d.points_ld;
                const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
                x = (float)(((m[0] * px + m[1] * py) + m[2] * pz) + m[3]);
            }
            d.d_xyz[i * d.xyz_ld + r] = x;
        }
    } else if (s == 2) {
        for (long long e = first; e < d.n * 3; e += step) {
            const long long i = e / 3;
            const int r = (int)(e - i * 3);
            const int o = model_of(d, d.d_index[i]);
            d.d_scale[i * d.scale_ld + r] = o >= 0 ? d.d_model_scale[3ll * o + r] : 0.0f;
        }
    } else {
        for (long long i = first; i < d.n; i += step) {
            const int o = model_of(d, d.d_index[i]);
            d.d_cls[i * d.cls_ld] = o >= 0 ? (long long)d.d_model_cls[o] : BACKGROUND_CLASS;
        }
    }
}

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
    const long long elems[4] = {d.n * fw, d.n * 3, d.n * 3, d.n};
    int total = 0;
    for (int s = 0; s < 4; ++s) {
        a.block_begin[s] = total;
        total += blocks_for(elems[s]);
    }
    a.block_begin[4] = total;
    scan_rows<<<total, 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    CV_LAUNCH_CHECK();
    return CV_OK;
}

size_t cv_sizeof_scan_rows_desc(void) { return sizeof(cv_scan_rows_desc); }

}  // extern "C"
