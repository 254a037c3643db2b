// Training-input staging (the half that sits on the training step's critical path): the reference's
// transform_train (dataset/nuscenes_dataset_torch_new.py:237-412) for transform_mode "sparse-to-dense", sparsifier "radar", modality
// rgbd / rgb, on the GPU and bit-identical to it for the same random draws.  Per frame the reference runs
//   depth : int16/256 -> /float32(scale) -> scipy.ndimage.rotate(order 0) -> Pillow NEAREST resize -> crop -> flip   (lidar, radar)
//   rgb   : rotate(order 0) per plane -> scipy.misc.imresize = byte scaling by the frame's min / max + Pillow BILINEAR resize on
//           8-bit data (horizontal pass, uint8 intermediate, vertical pass) -> crop -> flip -> ImageEnhance Brightness / Contrast /
//           Color in a drawn order -> /255
// Every step but two is a per-pixel gather, so nothing but the cropped window is ever computed; the two frame-wide scalars (the
// rotated frame's min / max, the crop's luma sum the Contrast enhancer needs) cut the work into three launches per chunk of frames:
//   train_minmax_kernel    min / max of the rotated RGB frame                                        -> stats (atomicMax, integers)
//   train_resample_kernel  rotate + byte scaling + 2x2-tap bilinear + crop + flip -> uint8x4 window; luma sum of the window with
//                          the enhancers that precede Contrast in this frame's order applied         -> stats (atomicAdd, integer)
//   train_finish_kernel    the three enhancers, the /255 table, both depth planes, planar fp32 stores (four pixels per thread)
// Integer reductions only, so the result does not depend on the order of the atomics; one atomic per workgroup and scalar (one per
// wave, every wave of a frame on the same word, cost 1.3 ms of a 1.45 ms batch at b=16 450x800).  No host synchronisation: per-frame
// parameters travel as kernel arguments (chunks of RD_STAGE_TRAIN_CHUNK frames), the (in, out)-dependent resize tables are device
// arrays.
//
// Arithmetic that must match the reference's rounding: rotation coordinates in float64 and the enhancers' blend in float32 with
// separate multiply and add (contraction is off for the whole file); the depth's float32 division through float64 (53 >= 2*24+2
// bits: rounding the correctly rounded double quotient to float is the correctly rounded float quotient); 255/(max-min) and v/255
// come from host-built tables (IEEE division on the host, as numpy does it).  With scale >= 1 Pillow's bilinear filter has at most two
// taps per axis, which is why the tables carry (first index, k0, k1).  Table indices are clamped to the frame before use, so a wrong
// table gives wrong pixels, never an out-of-bounds read.
#include "staging_geom.h"      // kChunk, TrainFrames, rot_src, near_src (shared with radar_filter.hip)

#include <algorithm>

#pragma clang fp contract(off)

namespace rd {

struct TrainLut { float v[256]; };

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// stats per frame: [0] 255 - min, [1] max (both by atomicMax from zero), [2..3] the 64-bit luma sum
__global__ __launch_bounds__(256) void train_minmax_kernel(const uint8_t* __restrict__ rgb, int H0, int W0, int b0, unsigned* __restrict__ stats,
                                                           const TrainFrames fr) {
    const int bl = blockIdx.y, b = b0 + bl;
    const double m00 = fr.f[bl].rot[0], m01 = fr.f[bl].rot[1], off0 = fr.f[bl].rot[2], m10 = fr.f[bl].rot[3], m11 = fr.f[bl].rot[4],
                 off1 = fr.f[bl].rot[5];
    const uint8_t* src = rgb + (int64_t)b * H0 * W0 * 3;
    const int n = H0 * W0;
    int inv_mn = 0, mx = 0;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const int y = e / W0, x = e - y * W0;
        int iy, ix;
        if (rot_src(m00, m01, off0, m10, m11, off1, H0, W0, y, x, iy, ix)) {
            const uint8_t* p = src + ((int64_t)iy * W0 + ix) * 3;
            const int r = p[0], g = p[1], bb = p[2];
            inv_mn = max(inv_mn, 255 - min(r, min(g, bb)));
            mx = max(mx, max(r, max(g, bb)));
        } else {
            inv_mn = 255;
        }
    }
    // one atomic pair per workgroup: every workgroup of a frame hits the same two words
    __shared__ int s_red[4][2];
    inv_mn = wave_max_i(inv_mn);
    mx = wave_max_i(mx);
    if ((threadIdx.x & 63) == 0) {
        s_red[threadIdx.x >> 6][0] = inv_mn;
        s_red[threadIdx.x >> 6][1] = mx;
    }
    rd_sync();
    if (threadIdx.x == 0) {
        atomicMax(stats + (int64_t)b * 4, (unsigned)max(max(s_red[0][0], s_red[1][0]), max(s_red[2][0], s_red[3][0])));
        atomicMax(stats + (int64_t)b * 4 + 1, (unsigned)max(max(s_red[0][1], s_red[1][1]), max(s_red[2][1], s_red[3][1])));
    }
}

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Pillow ImagingBlend on one byte: degenerate d, pixel p, factor f (float32); truncation inside [0, 1], clamp first outside
__device__ __forceinline__ int blend1(float d, int p, float f) {
    float t = d + f * ((float)p - d);
    if (!(f >= 0.f && f <= 1.f)) t = t <= 0.f ? 0.f : (t >= 255.f ? 255.f : t);
    return (int)t;
}

// one ImageEnhance step on an RGB pixel: 0 Brightness (black), 1 Contrast (the constant mean), 2 Color (the pixel's luma)
__device__ __forceinline__ void enhance1(int which, float f, float mean, int& r, int& g, int& b) {
    const float d = which == 0 ? 0.f : (which == 1 ? mean : (float)luma(r, g, b));
    r = blend1(d, r, f);
    g = blend1(d, g, f);
    b = blend1(d, b, f);
}

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void train_resample_kernel(const uint8_t* __restrict__ rgb, int H0, int W0, int ch, int cw, int b0,
                                                             const int4* __restrict__ bil_y, const int4* __restrict__ bil_x,
                                                             unsigned* __restrict__ stats, uchar4* __restrict__ mid, const TrainLut sc,
                                                             const TrainFrames fr) {
    __shared__ uint8_t s_map[256];
    const int bl = blockIdx.y, b = b0 + bl;
    {   // scipy <= 1.2 bytescale of this frame as a byte -> byte map
        const int mn = 255 - (int)stats[(int64_t)b * 4], mx = (int)stats[(int64_t)b * 4 + 1];
        const int cs = mx > mn ? mx - mn : 1;
        float t = ((float)(int)threadIdx.x - (float)mn) * sc.v[cs & 255];
        t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
        s_map[threadIdx.x] = (uint8_t)(int)(t + 0.5f);
    }
    rd_sync();
    const double m00 = fr.f[bl].rot[0], m01 = fr.f[bl].rot[1], off0 = fr.f[bl].rot[2], m10 = fr.f[bl].rot[3], m11 = fr.f[bl].rot[4],
                 off1 = fr.f[bl].rot[5];
    const int flip = fr.f[bl].flip;
    // the enhancers in front of Contrast in this frame's order
    int pre0 = -1, pre1 = -1;
    if (fr.f[bl].order[0] != 1) {
        pre0 = fr.f[bl].order[0];
        if (fr.f[bl].order[1] != 1) pre1 = fr.f[bl].order[1];
    }
    const float f0 = pre0 >= 0 ? fr.f[bl].factor[pre0] : 1.f, f1 = pre1 >= 0 ? fr.f[bl].factor[pre1] : 1.f;
    const uint8_t* src = rgb + (int64_t)b * H0 * W0 * 3;
    const uint8_t zero = s_map[0];
    const int n = ch * cw;
    unsigned lsum = 0;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const int y = e / cw, x = e - y * cw;
        const int4 ty = bil_y[(int64_t)b * ch + y], tx = bil_x[(int64_t)b * cw + (flip ? cw - 1 - x : x)];
        const int r0 = min(max(ty.x, 0), H0 - 1), r1 = min(r0 + 1, H0 - 1);
        const int c0 = min(max(tx.x, 0), W0 - 1), c1 = min(c0 + 1, W0 - 1);
        int h[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int p[2][3];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                int iy, ix;
                if (rot_src(m00, m01, off0, m10, m11, off1, H0, W0, i ? r1 : r0, j ? c1 : c0, iy, ix)) {
                    const uint8_t* q = src + ((int64_t)iy * W0 + ix) * 3;
                    p[j][0] = s_map[q[0]]; p[j][1] = s_map[q[1]]; p[j][2] = s_map[q[2]];
                } else {
                    p[j][0] = p[j][1] = p[j][2] = zero;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) h[i][c] = clip8(((1 << 21) + p[0][c] * tx.y + p[1][c] * tx.z) >> 22);
        }
        int r = clip8(((1 << 21) + h[0][0] * ty.y + h[1][0] * ty.z) >> 22);
        int g = clip8(((1 << 21) + h[0][1] * ty.y + h[1][1] * ty.z) >> 22);
        int bb = clip8(((1 << 21) + h[0][2] * ty.y + h[1][2] * ty.z) >> 22);
        mid[((int64_t)b * ch + y) * cw + x] = make_uchar4((uint8_t)r, (uint8_t)g, (uint8_t)bb, 0);
        if (pre0 >= 0) enhance1(pre0, f0, 0.f, r, g, bb);
        if (pre1 >= 0) enhance1(pre1, f1, 0.f, r, g, bb);
        lsum += (unsigned)luma(r, g, bb);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o, 64);
    __shared__ unsigned s_sum[4];
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = lsum;
    rd_sync();
    if (threadIdx.x == 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(stats + (int64_t)b * 4 + 2),
                  (unsigned long long)s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]);
}

__device__ __forceinline__ float depth_px(const int16_t* __restrict__ d, int64_t idx, bool ok, double div) {
    if (!ok) return 0.f;
    const float v = (float)d[idx] * (1.0f / 256.0f);                 // int16 / 256. is exact in float32
    return (float)((double)v / div);                                // == the correctly rounded float32 quotient (see the header)
}

__global__ __launch_bounds__(256) void train_finish_kernel(const int16_t* __restrict__ lidar, const int16_t* __restrict__ radar, int H0, int W0,
                                                           int ch, int cw, int b0, const int32_t* __restrict__ near_y,
                                                           const int32_t* __restrict__ near_x, const unsigned* __restrict__ stats,
                                                           const uchar4* __restrict__ mid, float max_depth, int cin,
                                                           float* __restrict__ inputs, float* __restrict__ labels, const TrainLut lut,
                                                           const TrainFrames fr) {
    __shared__ float s_lut[256];
    s_lut[threadIdx.x] = lut.v[threadIdx.x];
    rd_sync();
    const int bl = blockIdx.y, b = b0 + bl;
    const double m00 = fr.f[bl].rot[0], m01 = fr.f[bl].rot[1], off0 = fr.f[bl].rot[2], m10 = fr.f[bl].rot[3], m11 = fr.f[bl].rot[4],
                 off1 = fr.f[bl].rot[5];
    const int flip = fr.f[bl].flip;
    const int o0 = fr.f[bl].order[0], o1 = fr.f[bl].order[1], o2 = fr.f[bl].order[2];
    const float f0 = fr.f[bl].factor[o0], f1 = fr.f[bl].factor[o1], f2 = fr.f[bl].factor[o2];
    const double div = (double)(float)fr.f[bl].scale;              // lidar_depth /= float(scale): a float32 array by a float32 scalar
    const int64_t plane = (int64_t)ch * cw;
    // ImageStat mean of the luma image, int(mean + 0.5): (2 sum + N) / 2N in integers (mean + 0.5 is never within an ulp of an integer
    // unless it is one: the nearest miss is 1/(2N))
    const unsigned long long ls = *reinterpret_cast<const unsigned long long*>(stats + (int64_t)b * 4 + 2);
    const float mean = (float)(int)((2ull * ls + (unsigned long long)plane) / (2ull * (unsigned long long)plane));
    const int16_t* lid = lidar + (int64_t)b * H0 * W0;
    const int16_t* rad = radar ? radar + (int64_t)b * H0 * W0 : nullptr;
    const uchar4* mid_b = mid + (int64_t)b * plane;
    const int W4 = (cw + 3) >> 2, n = ch * W4;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const int y = e / W4, x0 = (e - y * W4) * 4, nx = min(4, cw - x0);
        const int sy = near_src(near_y, b, ch, y, H0);
        float o[5][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < nx) {
                const uchar4 px = mid_b[(int64_t)y * cw + x0 + k];
                int r = px.x, g = px.y, bb = px.z;
                enhance1(o0, f0, mean, r, g, bb);
                enhance1(o1, f1, mean, r, g, bb);
                enhance1(o2, f2, mean, r, g, bb);
                o[0][k] = s_lut[r]; o[1][k] = s_lut[g]; o[2][k] = s_lut[bb];
                const int x = x0 + k;
                const int sx = near_src(near_x, b, cw, flip ? cw - 1 - x : x, W0);
                int iy, ix;
                const bool ok = rot_src(m00, m01, off0, m10, m11, off1, H0, W0, sy, sx, iy, ix);
                const int64_t idx = (int64_t)iy * W0 + ix;
                o[4][k] = depth_px(lid, idx, ok, div);
                const float rv = rad ? depth_px(rad, idx, ok, div) : 0.f;
                o[3][k] = rv > max_depth ? 0.f : rv;
            }
        }
        const int64_t dst = (int64_t)y * cw + x0;
        float* in_b = inputs + (int64_t)b * cin * plane + dst;
        float* lb = labels + (int64_t)b * plane + dst;
        if (nx == 4 && ((reinterpret_cast<uintptr_t>(in_b) | reinterpret_cast<uintptr_t>(lb) | (uintptr_t)(plane * 4)) & 15) == 0) {
            for (int c = 0; c < cin; ++c) {
                const float4 v = c == 0 ? make_float4(o[0][0], o[0][1], o[0][2], o[0][3])
                               : c == 1 ? make_float4(o[1][0], o[1][1], o[1][2], o[1][3])
                               : c == 2 ? make_float4(o[2][0], o[2][1], o[2][2], o[2][3])
                                        : make_float4(o[3][0], o[3][1], o[3][2], o[3][3]);
                *reinterpret_cast<float4*>(in_b + c * plane) = v;
            }
            *reinterpret_cast<float4*>(lb) = make_float4(o[4][0], o[4][1], o[4][2], o[4][3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < nx) {
                    in_b[k] = o[0][k]; in_b[plane + k] = o[1][k]; in_b[2 * plane + k] = o[2][k];
                    if (cin == 4) in_b[3 * plane + k] = o[3][k];
                    lb[k] = o[4][k];
                }
            }
        }
    }
}

static inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

}  // namespace rd
using namespace rd;

extern "C" int64_t rd_stage_train_workspace_bytes(int32_t B, int32_t H0, int32_t W0, int32_t ch, int32_t cw) {
    if (B <= 0 || H0 <= 0 || W0 <= 0 || ch <= 0 || cw <= 0 || H0 < ch || W0 < cw) {
        set_error("stage_train_workspace_bytes: B=%d frames %dx%d crop %dx%d", B, H0, W0, ch, cw);
        return RD_EINVAL;
    }
    return align256((int64_t)B * 16) + (int64_t)B * ch * cw * 4;      // stats, then the uint8x4 window
}

extern "C" int rd_stage_frames_train(const uint8_t* rgb_hwc, const int16_t* lidar, const int16_t* radar, int32_t B, int32_t H0, int32_t W0,
                                     int32_t ch, int32_t cw, const RdStageTrainFrame* frames, const int32_t* near_y, const int32_t* near_x,
                                     const int32_t* bil_y, const int32_t* bil_x, void* workspace, float max_depth, int32_t modality,
                                     float* inputs, float* labels, void* stream) {
    RD_CHECK_ARG(modality == RD_MODALITY_RGBD || modality == RD_MODALITY_RGB, "stage_frames_train: modality %d (0 rgbd, 1 rgb)", modality);
    RD_CHECK_ARG(rgb_hwc && lidar && (radar || modality == RD_MODALITY_RGB) && frames && near_y && near_x && bil_y && bil_x && workspace &&
                     inputs && labels, "stage_frames_train: null argument");
    RD_CHECK_ARG(B > 0 && ch > 0 && cw > 0 && H0 >= ch && W0 >= cw && (int64_t)H0 * W0 < (1ll << 30),
                 "stage_frames_train: crop %dx%d does not fit the %dx%d frame (B=%d)", ch, cw, H0, W0, B);
    RD_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 16 == 0 && reinterpret_cast<uintptr_t>(bil_y) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(bil_x) % 16 == 0, "stage_frames_train: workspace and bilinear tables must be 16-byte aligned");
    for (int b = 0; b < B; ++b) {
        const RdStageTrainFrame& f = frames[b];
        RD_CHECK_ARG(f.scale >= 1.0 && f.scale <= 64.0, "stage_frames_train: frame %d: scale %g below 1 (or above 64)", b, f.scale);
        const int oh = (int)((double)H0 * f.scale), ow = (int)((double)W0 * f.scale);       // imresize: (im.size * scale).astype(int)
        RD_CHECK_ARG(f.h_start >= 0 && f.w_start >= 0 && f.h_start + ch <= oh && f.w_start + cw <= ow,
                     "stage_frames_train: frame %d: crop window %dx%d at (%d,%d) outside the resized %dx%d frame", b, ch, cw, f.h_start,
                     f.w_start, oh, ow);
        int seen = 0;
        for (int k = 0; k < 3; ++k) seen |= (f.order[k] >= 0 && f.order[k] <= 2) ? 1 << f.order[k] : 8;
        RD_CHECK_ARG(seen == 7, "stage_frames_train: frame %d: jitter order (%d,%d,%d) is not a permutation of 0,1,2", b, f.order[0],
                     f.order[1], f.order[2]);
    }
    static TrainLut lut255, lutsc;
    static std::once_flag once;
    std::call_once(once, [] {
        for (int v = 0; v < 256; ++v) {
            lut255.v[v] = (float)((double)v / 255.0);                      // uint8 array / python float: float64, then astype(float32)
            lutsc.v[v] = (float)(255.0 / (double)(v ? v : 1));             // bytescale: float32(255.0 / float(cmax - cmin))
        }
    });
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned* stats = static_cast<unsigned*>(workspace);
    uchar4* mid = reinterpret_cast<uchar4*>(static_cast<char*>(workspace) + align256((int64_t)B * 16));
    RD_CHECK_HIP(hipMemsetAsync(stats, 0, (size_t)B * 16, s));
    const int cin = modality == RD_MODALITY_RGB ? 3 : 4;
    for (int b0 = 0; b0 < B; b0 += kChunk) {
        const int nb = std::min(kChunk, B - b0);
        // grid-stride kernels: 16 workgroups per CU over the chain's frames (one atomic per workgroup and frame-wide scalar)
        const int64_t cap = std::max(64, num_cus() * 16 / nb);
        const int g_a = (int)std::min(cdiv64((int64_t)H0 * W0, 256), cap);
        const int g_b = (int)std::min(cdiv64((int64_t)ch * cw, 256), cap);
        const int g_c = (int)std::min(cdiv64((int64_t)ch * ((cw + 3) / 4), 256), cap);
        TrainFrames fr;
        memset(&fr, 0, sizeof(fr));
        memcpy(fr.f, frames + b0, sizeof(RdStageTrainFrame) * nb);
        hipLaunchKernelGGL(train_minmax_kernel, dim3(g_a, nb), dim3(256), 0, s, rgb_hwc, H0, W0, b0, stats, fr);
        RD_CHECK_LAUNCH("train_minmax_kernel");
        hipLaunchKernelGGL(train_resample_kernel, dim3(g_b, nb), dim3(256), 0, s, rgb_hwc, H0, W0, ch, cw, b0,
                           reinterpret_cast<const int4*>(bil_y), reinterpret_cast<const int4*>(bil_x), stats, mid, lutsc, fr);
        RD_CHECK_LAUNCH("train_resample_kernel");
        hipLaunchKernelGGL(train_finish_kernel, dim3(g_c, nb), dim3(256), 0, s, lidar, radar, H0, W0, ch, cw, b0, near_y, near_x, stats, mid,
                           max_depth, cin, inputs, labels, lut255, fr);
        RD_CHECK_LAUNCH("train_finish_kernel");
    }
    return RD_OK;
}
