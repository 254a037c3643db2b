// The radar_filtered sparsifier on the GPU: what the reference's DataLoader worker does to every frame in filter_radar_points
// (dataset/nuscenes_dataset_torch_new.py:557-584) and what transform_val / transform_train then do with its results (:323-348,
// :462-486), for a batch of frames with ragged point counts.
//   radar_filter_kernel      filter_radar_points_gt (dataset/radar_preprocessing.py:77-122): per radar point the three nearest lidar
//                            points and the reference's two depth-aware thresholds -> label, valid, topk.  One wavefront per radar
//                            point: lanes stride over the frame's lidar points, each keeping its own sorted top three of
//                            (distance, index); three rounds of a wave-wide minimum merge them, the owning lane pops its head.  The
//                            reference sorts the whole [radar x lidar] matrix twice.
//   index_scatter_kernel     index_map: point i at (int)y, (int)x by integer atomicMax (the reference's repeated-index assignment
//                            keeps the last = highest index)
//   index_filter_val_kernel / index_filter_train_kernel
//                            index_map through the depth maps' transform (centre crop / NEAREST tables + order-0 rotation + crop +
//                            flip, staging_geom.h) and inputs[b,3] = 0 where the transformed index names a point the filter rejected
// Per-frame counts travel as launch arguments, RD_STAGE_TRAIN_CHUNK frames per launch; nothing at or beyond a count is read.  No
// barriers, no LDS, no floating-point atomics.
//
// Arithmetic that must match the reference: float64 throughout, dx*dx + dy*dy with separate multiplies and add (contraction is off
// for the whole file), IEEE sqrt and division; the log constants come from the host.  Only exp is the device library's; the
// fixture keeps every decision at least 1e-6 (relative) away from its threshold.
#include "staging_geom.h"

#include <algorithm>
#include <limits.h>

#pragma clang fp contract(off)

namespace rd {

struct RadarCounts { int32_t nr[kChunk], nl[kChunk]; };

constexpr int kNoIndex = INT_MAX;       // the index of an empty top-three slot: sorts after every lidar point at the same distance

__device__ __forceinline__ bool before(double d, int i, double e, int j) { return d < e || (d == e && i < j); }

__global__ __launch_bounds__(256) void radar_filter_kernel(const double* __restrict__ rxy, const double* __restrict__ rdep,
                                                           const double* __restrict__ lxy, const double* __restrict__ ldep, int b0, int Rmax,
                                                           int Lmax, double dist_log, double dist_off, double depth_log, double depth_off,
                                                           uint8_t* __restrict__ labels, uint8_t* __restrict__ valid,
                                                           int32_t* __restrict__ topk, const RadarCounts cnt) {
    const int bl = blockIdx.y, b = b0 + bl;
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= Rmax) return;                                      // wave-uniform, and the kernel has no barrier
    const int nr = cnt.nr[bl], nl = cnt.nl[bl];
    const int64_t row = (int64_t)b * Rmax + r;
    if (r >= nr) {
        if (lane == 0) labels[row] = 0, valid[row] = 0;
        if (lane < 3) topk[row * 3 + lane] = -1;
        return;
    }
    const double px = rxy[row * 2], py = rxy[row * 2 + 1];
    const double inf = __builtin_huge_val();
    double d0 = inf, d1 = inf, d2 = inf;
    int i0 = kNoIndex, i1 = kNoIndex, i2 = kNoIndex;
    const double* lx = lxy + (int64_t)b * Lmax * 2;
    for (int j = lane; j < nl; j += 64) {
        const double dx = px - lx[2 * j], dy = py - lx[2 * j + 1];
        const double d = sqrt(dx * dx + dy * dy);
        if (before(d, j, d2, i2)) {                              // (a NaN distance is never before anything: it is left out)
            if (before(d, j, d1, i1)) {
                d2 = d1, i2 = i1;
                if (before(d, j, d0, i0)) {
                    d1 = d0, i1 = i0, d0 = d, i0 = j;
                } else {
                    d1 = d, i1 = j;
                }
            } else {
                d2 = d, i2 = j;
            }
        }
    }
    double wd[3];
    int wi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double md = d0;
        int mi = i0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(md, o, 64);
            const int oi = __shfl_xor(mi, o, 64);
            if (before(od, oi, md, mi)) md = od, mi = oi;
        }
        wd[k] = md, wi[k] = mi;
        if (mi != kNoIndex && i0 == mi) d0 = d1, i0 = i1, d1 = d2, i1 = i2, d2 = inf, i2 = kNoIndex;      // lidar indices are unique: one owner
    }
    if (lane != 0) return;
    const double rd_ = rdep[row];
    const double* ld = ldep + (int64_t)b * Lmax;
    int c = 0;
    double dep[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bool have = wi[k] >= 0 && wi[k] < nl;              // fewer than three comparable distances (NaN coordinates): no read
        dep[k] = have ? ld[wi[k]] : 0.0;
        c += have && wd[k] <= exp(dep[k] * dist_log / 100.0 + dist_off);
    }
    int pass = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const bool have = wi[k] >= 0 && wi[k] < nl;
        pass += k < c && have && rd_ - dep[k] < exp(dep[k] * depth_log / 100.0 + depth_off);
    }
    const int label = c == 0 ? 2 : (pass >= (c + 1) / 2 ? 1 : 0);
    labels[row] = (uint8_t)label;
    valid[row] = label > 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) topk[row * 3 + k] = (wi[k] >= 0 && wi[k] < nl) ? wi[k] : -1;
}

__global__ __launch_bounds__(256) void index_scatter_kernel(const double* __restrict__ rxy, int b0, int Rmax, int H0, int W0,
                                                            int32_t* __restrict__ map, const RadarCounts cnt) {
    const int bl = blockIdx.y, b = b0 + bl;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt.nr[bl]) return;
    const double px = rxy[((int64_t)b * Rmax + i) * 2], py = rxy[((int64_t)b * Rmax + i) * 2 + 1];
    // truncation toward zero: (-1, 0) goes to 0 as astype(np.int32) sends it; NaN fails every comparison
    if (!(px > -1.0 && px < (double)W0 && py > -1.0 && py < (double)H0)) return;
    atomicMax(map + ((int64_t)b * H0 + (int)py) * W0 + (int)px, i);
}

// the filter on one staged pixel: the transformed index names a point of this frame that the filter rejected
__device__ __forceinline__ bool rejected(int v, int nr, const uint8_t* __restrict__ valid_b) { return v >= 0 && v < nr && valid_b[v] == 0; }

__global__ __launch_bounds__(256) void index_filter_val_kernel(const int32_t* __restrict__ map, const uint8_t* __restrict__ valid, int b0, int Rmax,
                                                               int H0, int W0, int i0, int j0, int H, int W, int apply,
                                                               float* __restrict__ inputs, int32_t* __restrict__ out, const RadarCounts cnt) {
    const int bl = blockIdx.y, b = b0 + bl, nr = cnt.nr[bl], n = H * W;
    const int32_t* src = map + (int64_t)b * H0 * W0;
    const uint8_t* valid_b = valid + (int64_t)b * Rmax;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const int y = e / W, x = e - y * W;
        const int v = src[(int64_t)(i0 + y) * W0 + j0 + x];
        out[(int64_t)b * n + e] = v;
        if (apply && rejected(v, nr, valid_b)) inputs[((int64_t)b * 4 + 3) * n + e] = 0.f;
    }
}

__global__ __launch_bounds__(256) void index_filter_train_kernel(const int32_t* __restrict__ map, const uint8_t* __restrict__ valid, int b0,
                                                                 int Rmax, int H0, int W0, int ch, int cw, const int32_t* __restrict__ near_y,
                                                                 const int32_t* __restrict__ near_x, int apply, float* __restrict__ inputs,
                                                                 int32_t* __restrict__ out, const RadarCounts cnt, const TrainFrames fr) {
    const int bl = blockIdx.y, b = b0 + bl, nr = cnt.nr[bl], n = ch * cw;
    const double m00 = fr.f[bl].rot[0], m01 = fr.f[bl].rot[1], off0 = fr.f[bl].rot[2], m10 = fr.f[bl].rot[3], m11 = fr.f[bl].rot[4],
                 off1 = fr.f[bl].rot[5];
    const int flip = fr.f[bl].flip;
    const int32_t* src = map + (int64_t)b * H0 * W0;
    const uint8_t* valid_b = valid + (int64_t)b * Rmax;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const int y = e / cw, x = e - y * cw;
        const int sy = near_src(near_y, b, ch, y, H0), sx = near_src(near_x, b, cw, flip ? cw - 1 - x : x, W0);
        int iy, ix;
        const bool ok = rot_src(m00, m01, off0, m10, m11, off1, H0, W0, sy, sx, iy, ix);
        const int v = ok ? src[(int64_t)iy * W0 + ix] : 0;       // the rotation's cval: 0, which is also point 0's index
        out[(int64_t)b * n + e] = v;
        if (apply && rejected(v, nr, valid_b)) inputs[((int64_t)b * 4 + 3) * n + e] = 0.f;
    }
}

static int check_counts(const char* what, const int32_t* n_radar, const int32_t* n_lidar, int B, int Rmax, int Lmax) {
    for (int b = 0; b < B; ++b) {
        RD_CHECK_CODE(n_radar[b] >= 0 && n_radar[b] <= Rmax, RD_ERADAR_NRADAR, "%s: frame %d: n_radar %d outside 0..Rmax=%d", what, b, n_radar[b], Rmax);
        if (!n_lidar) continue;
        RD_CHECK_CODE(n_lidar[b] >= 0 && n_lidar[b] <= Lmax, RD_ERADAR_NLIDAR, "%s: frame %d: n_lidar %d outside 0..Lmax=%d", what, b, n_lidar[b], Lmax);
        RD_CHECK_CODE(n_radar[b] == 0 || n_lidar[b] >= 3, RD_ERADAR_FEWLIDAR,
                      "%s: frame %d: %d radar points but %d lidar points: three neighbours are needed", what, b, n_radar[b], n_lidar[b]);
    }
    return RD_OK;
}

static RadarCounts chunk_counts(const int32_t* n_radar, const int32_t* n_lidar, int b0, int nb) {
    RadarCounts c;
    memset(&c, 0, sizeof(c));
    for (int i = 0; i < nb; ++i) {
        c.nr[i] = n_radar[b0 + i];
        if (n_lidar) c.nl[i] = n_lidar[b0 + i];
    }
    return c;
}

static inline bool batch_ok(int B, int Rmax) { return B >= 1 && B <= 65536 && Rmax >= 1 && Rmax <= (1 << 20); }
static inline bool frame_ok(int H0, int W0) { return H0 >= 1 && W0 >= 1 && (int64_t)H0 * W0 < (1ll << 30); }

}  // namespace rd
using namespace rd;

extern "C" int rd_radar_filter_points(const double* radar_xy, const double* radar_depth, const double* lidar_xy, const double* lidar_depth,
                                      const int32_t* n_radar, const int32_t* n_lidar, int32_t B, int32_t Rmax, int32_t Lmax,
                                      const double* thresholds, uint8_t* labels, uint8_t* valid, int32_t* topk, void* stream) {
    RD_CHECK_CODE(radar_xy && radar_depth && lidar_xy && lidar_depth && n_radar && n_lidar && thresholds && labels && valid && topk,
                  RD_ERADAR_NULL, "radar_filter_points: null argument");
    RD_CHECK_CODE(batch_ok(B, Rmax) && Lmax >= 1 && Lmax <= (1 << 24), RD_ERADAR_RANGE,
                  "radar_filter_points: B=%d (1..65536) Rmax=%d (1..2^20) Lmax=%d (1..2^24)", B, Rmax, Lmax);
    if (const int rc = check_counts("radar_filter_points", n_radar, n_lidar, B, Rmax, Lmax)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int b0 = 0; b0 < B; b0 += kChunk) {
        const int nb = std::min(kChunk, B - b0);
        hipLaunchKernelGGL(radar_filter_kernel, dim3(cdiv(Rmax, 4), nb), dim3(256), 0, s, radar_xy, radar_depth, lidar_xy, lidar_depth, b0, Rmax,
                           Lmax, thresholds[0], thresholds[1], thresholds[2], thresholds[3], labels, valid, topk,
                           chunk_counts(n_radar, n_lidar, b0, nb));
        RD_CHECK_LAUNCH("radar_filter_kernel");
    }
    return RD_OK;
}

extern "C" int rd_radar_index_map(const double* radar_xy, const int32_t* n_radar, int32_t B, int32_t Rmax, int32_t H0, int32_t W0,
                                  int32_t* index_map, void* stream) {
    RD_CHECK_CODE(radar_xy && n_radar && index_map, RD_ERADAR_NULL, "radar_index_map: null argument");
    RD_CHECK_CODE(batch_ok(B, Rmax) && frame_ok(H0, W0), RD_ERADAR_RANGE, "radar_index_map: B=%d (1..65536) Rmax=%d (1..2^20) frame %dx%d (below 2^30 pixels)",
                  B, Rmax, H0, W0);
    if (const int rc = check_counts("radar_index_map", n_radar, nullptr, B, Rmax, 0)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    RD_CHECK_HIP(hipMemsetAsync(index_map, 0xFF, (size_t)B * H0 * W0 * sizeof(int32_t), s));          // every byte 0xFF: int32 -1
    for (int b0 = 0; b0 < B; b0 += kChunk) {
        const int nb = std::min(kChunk, B - b0);
        hipLaunchKernelGGL(index_scatter_kernel, dim3(cdiv(Rmax, 256), nb), dim3(256), 0, s, radar_xy, b0, Rmax, H0, W0, index_map,
                           chunk_counts(n_radar, nullptr, b0, nb));
        RD_CHECK_LAUNCH("index_scatter_kernel");
    }
    return RD_OK;
}

extern "C" int rd_stage_index_filter_val(const int32_t* index_map, const uint8_t* valid, const int32_t* n_radar, int32_t B, int32_t Rmax,
                                         int32_t H0, int32_t W0, int32_t i0, int32_t j0, int32_t H, int32_t W, int32_t apply_filter,
                                         float* inputs, int32_t* index_map_out, void* stream) {
    RD_CHECK_CODE(index_map && valid && n_radar && index_map_out && (inputs || !apply_filter), RD_ERADAR_NULL, "stage_index_filter_val: null argument");
    RD_CHECK_CODE(batch_ok(B, Rmax) && frame_ok(H0, W0), RD_ERADAR_RANGE,
                  "stage_index_filter_val: B=%d (1..65536) Rmax=%d (1..2^20) frame %dx%d (below 2^30 pixels)", B, Rmax, H0, W0);
    if (const int rc = check_counts("stage_index_filter_val", n_radar, nullptr, B, Rmax, 0)) return rc;
    RD_CHECK_CODE(H > 0 && W > 0 && i0 >= 0 && j0 >= 0 && i0 + H <= H0 && j0 + W <= W0, RD_ERADAR_CROP,
                  "stage_index_filter_val: crop %dx%d at (%d,%d) does not fit the %dx%d frame", H, W, i0, j0, H0, W0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int b0 = 0; b0 < B; b0 += kChunk) {
        const int nb = std::min(kChunk, B - b0);
        const int g = (int)std::min(cdiv64((int64_t)H * W, 256), (int64_t)std::max(64, num_cus() * 16 / nb));
        hipLaunchKernelGGL(index_filter_val_kernel, dim3(g, nb), dim3(256), 0, s, index_map, valid, b0, Rmax, H0, W0, i0, j0, H, W,
                           apply_filter ? 1 : 0, inputs, index_map_out, chunk_counts(n_radar, nullptr, b0, nb));
        RD_CHECK_LAUNCH("index_filter_val_kernel");
    }
    return RD_OK;
}

extern "C" int rd_stage_index_filter_train(const int32_t* index_map, const uint8_t* valid, const int32_t* n_radar, int32_t B, int32_t Rmax,
                                           int32_t H0, int32_t W0, int32_t ch, int32_t cw, const RdStageTrainFrame* frames,
                                           const int32_t* near_y, const int32_t* near_x, int32_t apply_filter, float* inputs,
                                           int32_t* index_map_out, void* stream) {
    RD_CHECK_CODE(index_map && valid && n_radar && frames && near_y && near_x && index_map_out && (inputs || !apply_filter), RD_ERADAR_NULL,
                  "stage_index_filter_train: null argument");
    RD_CHECK_CODE(batch_ok(B, Rmax) && frame_ok(H0, W0), RD_ERADAR_RANGE,
                  "stage_index_filter_train: B=%d (1..65536) Rmax=%d (1..2^20) frame %dx%d (below 2^30 pixels)", B, Rmax, H0, W0);
    if (const int rc = check_counts("stage_index_filter_train", n_radar, nullptr, B, Rmax, 0)) return rc;
    RD_CHECK_CODE(ch > 0 && cw > 0 && H0 >= ch && W0 >= cw, RD_ERADAR_CROP, "stage_index_filter_train: crop %dx%d does not fit the %dx%d frame", ch,
                  cw, H0, W0);
    for (int b = 0; b < B; ++b) {
        const RdStageTrainFrame& f = frames[b];
        RD_CHECK_CODE(f.scale >= 1.0 && f.scale <= 64.0, RD_ERADAR_CROP, "stage_index_filter_train: frame %d: scale %g below 1 (or above 64)", b, f.scale);
        const int oh = (int)((double)H0 * f.scale), ow = (int)((double)W0 * f.scale);       // imresize: (im.size * scale).astype(int)
        RD_CHECK_CODE(f.h_start >= 0 && f.w_start >= 0 && f.h_start + ch <= oh && f.w_start + cw <= ow, RD_ERADAR_CROP,
                      "stage_index_filter_train: frame %d: crop window %dx%d at (%d,%d) outside the resized %dx%d frame", b, ch, cw, f.h_start,
                      f.w_start, oh, ow);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int b0 = 0; b0 < B; b0 += kChunk) {
        const int nb = std::min(kChunk, B - b0);
        const int g = (int)std::min(cdiv64((int64_t)ch * cw, 256), (int64_t)std::max(64, num_cus() * 16 / nb));
        TrainFrames fr;
        memset(&fr, 0, sizeof(fr));
        memcpy(fr.f, frames + b0, sizeof(RdStageTrainFrame) * nb);
        hipLaunchKernelGGL(index_filter_train_kernel, dim3(g, nb), dim3(256), 0, s, index_map, valid, b0, Rmax, H0, W0, ch, cw, near_y, near_x,
                           apply_filter ? 1 : 0, inputs, index_map_out, chunk_counts(n_radar, nullptr, b0, nb), fr);
        RD_CHECK_LAUNCH("index_filter_train_kernel");
    }
    return RD_OK;
}
