// The validation comparison rows on the GPU (the reference: utils.py:114-153, merge_into_row / merge_into_row_with_gt /
// colored_depthmap, as save_image's astype('uint8') leaves them): [rgb | depth planes...] side by side, H x kW x 3 uint8.
//   range_kernel        per frame the float32 minimum and maximum over all of the frame's depth planes together: grid-stride loads
//                       (16-byte ones where every plane allows), a wave-wide reduction, the four waves' values through LDS, then one
//                       integer atomicMax per workgroup and bound on an order-preserving integer key of the float.  The minimum is
//                       kept as the maximum of the complemented key, so one memset of zeros starts both.  Integer atomics only: the
//                       pair does not depend on the order of arrival.  Skipped when the caller gives the range.
//   render_kernel       one streaming pass.  A workgroup walks rows of one frame; a thread owns one ALIGNED dword of the output row,
//                       which always spans two neighbouring pixels of the row: it colours both, joins the six bytes and shifts the
//                       four it owns into place.  A row's first and last dword may be partly outside the row (odd width, odd panel
//                       count, a canvas row that starts on an odd byte): those are written byte by byte, nothing outside the row is
//                       touched.  The 259 colours sit in LDS as packed words, filled once per workgroup.
// Index of a depth pixel (matplotlib's Colormap.__call__ on a float32 array): rel = (d - d_min) / denom with a correctly rounded float32
// division, xa = rel * 256; xa == 256 -> 255, xa < 0 -> 256 (under), xa >= 256 -> 257 (over), NaN -> 258 (bad), else trunc(xa).
// Contraction is off for the whole file and the division is __fdiv_rn.
#include "common.h"

#include <algorithm>
#include <math.h>

#pragma clang fp contract(off)

namespace rd {

constexpr int kVisBlock = 256;                      // threads of both launches: four wavefronts (range_kernel's part[] relies on it)
constexpr int kLutRows = 259;                       // 256 colours, under, over, bad

struct VisPlanes {                                  // by value in the kernel arguments; only ever indexed with constants
    const float* p[3];
    int64_t stride[3];                              // elements between frames
    int count;
};

// Order-preserving key of a float: a < b  <=>  key(a) < key(b) as unsigned integers (-0 sorts just below +0).
__device__ __forceinline__ uint32_t float_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

template <bool VEC>
__global__ __launch_bounds__(kVisBlock) void range_kernel(const VisPlanes pl, int n, uint32_t* __restrict__ range) {
    __shared__ float part[2][kVisBlock / 64];
    static_assert(kVisBlock == 256, "the reduction below reads four partial values");
    const int b = blockIdx.y;
    float lo = INFINITY, hi = -INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k >= pl.count) continue;                                            // uniform
        const float* pb = pl.p[k] + (int64_t)b * pl.stride[k];
        if (VEC) {                                                              // n % 4 == 0 and every frame 16-byte aligned (host)
            const float4* p4 = reinterpret_cast<const float4*>(pb);
#pragma unroll 4
            for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < (n >> 2); e += gridDim.x * blockDim.x) {
                const float4 v = p4[e];
                lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
                hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
            }
        } else {
#pragma unroll 4
            for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
                const float v = pb[e];
                lo = fminf(lo, v), hi = fmaxf(hi, v);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = fminf(lo, __shfl_xor(lo, o, 64)), hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    if ((threadIdx.x & 63) == 0) part[0][threadIdx.x >> 6] = lo, part[1][threadIdx.x >> 6] = hi;
    rd_sync();                                                                  // reached by every thread of the block
    if (threadIdx.x != 0) return;
    lo = fminf(fminf(part[0][0], part[0][1]), fminf(part[0][2], part[0][3]));
    hi = fmaxf(fmaxf(part[1][0], part[1][1]), fmaxf(part[1][2], part[1][3]));
    if (lo > hi) return;                                                        // a block that saw no pixel
    atomicMax(&range[2 * b], ~float_key(lo));
    atomicMax(&range[2 * b + 1], float_key(hi));
}

__device__ __forceinline__ int color_index(float d, float lo, float denom) {
    const float xa = __fdiv_rn(d - lo, denom) * 256.f;
    if (xa != xa) return 258;
    if (xa == 256.f) return 255;
    if (xa < 0.f) return 256;
    if (xa >= 256.f) return 257;
    return (int)xa;
}

// the three bytes of pixel m of the row (0 <= m < k*W; anything else gives 0 and reads nothing): R | G << 8 | B << 16
__device__ __forceinline__ uint32_t row_pixel(int m, int W, int kW, int64_t row_off, int64_t n, const float* __restrict__ rgb, const float* p0,
                                              const float* p1, const float* p2, float lo, float denom, const uint32_t* lut) {
    if (m < 0 || m >= kW) return 0u;
    int panel = (m >= W) + (m >= 2 * W) + (m >= 3 * W);
    const int64_t at = row_off + (m - panel * W);
    if (rgb) {
        if (panel == 0) {
            const uint32_t r = (uint32_t)(int)(255.f * rgb[at]) & 0xffu, g = (uint32_t)(int)(255.f * rgb[n + at]) & 0xffu,
                           bl = (uint32_t)(int)(255.f * rgb[2 * n + at]) & 0xffu;
            return r | (g << 8) | (bl << 16);
        }
        --panel;
    }
    const float* p = panel == 0 ? p0 : panel == 1 ? p1 : p2;
    return lut[color_index(p[at], lo, denom)];
}

__global__ __launch_bounds__(kVisBlock) void render_kernel(const float* __restrict__ rgb, int64_t rgb_stride, const VisPlanes pl, int H, int W,
                                                        const uint32_t* __restrict__ range, float lo_given, float denom_given,
                                                        const uint8_t* __restrict__ table, uint8_t* __restrict__ out, int64_t frame_stride,
                                                        int64_t row_pitch) {
    __shared__ uint32_t lut[kLutRows + 1];
    for (int t = threadIdx.x; t < kLutRows; t += blockDim.x)
        lut[t] = (uint32_t)table[3 * t] | ((uint32_t)table[3 * t + 1] << 8) | ((uint32_t)table[3 * t + 2] << 16);
    rd_sync();                                                                  // reached by every thread of the block
    const int b = blockIdx.y;
    float lo = lo_given, denom = denom_given;
    if (range) {
        lo = key_float(~range[2 * b]);
        denom = key_float(range[2 * b + 1]) - lo;
    }
    const int64_t n = (int64_t)H * W;
    const float* rb = rgb ? rgb + (int64_t)b * rgb_stride : nullptr;
    const float* p0 = pl.p[0] + (int64_t)b * pl.stride[0];
    const float* p1 = pl.count > 1 ? pl.p[1] + (int64_t)b * pl.stride[1] : p0;
    const float* p2 = pl.count > 2 ? pl.p[2] + (int64_t)b * pl.stride[2] : p0;
    const int kW = (pl.count + (rgb ? 1 : 0)) * W, L = 3 * kW;                  // pixels and bytes of an output row
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        uint8_t* row = out + (int64_t)b * frame_stride + (int64_t)y * row_pitch;
        const int a0 = (int)(reinterpret_cast<uintptr_t>(row) & 3);            // the row starts a0 bytes into its first dword
        const int ndw = (a0 + L + 3) >> 2;
        const int64_t row_off = (int64_t)y * W;
        for (int i = threadIdx.x; i < ndw; i += blockDim.x) {
            const int q0 = 4 * i - a0;                                          // row byte of this dword's byte 0: -3 .. L-1
            const int m0 = (q0 + 3) / 3 - 1, sh = (q0 + 3) - 3 * (m0 + 1);     // q0 = 3 * m0 + sh, m0 >= -1
            const uint32_t c0 = row_pixel(m0, W, kW, row_off, n, rb, p0, p1, p2, lo, denom, lut);
            const uint32_t c1 = row_pixel(m0 + 1, W, kW, row_off, n, rb, p0, p1, p2, lo, denom, lut);
            const uint32_t dw = (uint32_t)(((unsigned long long)c0 | ((unsigned long long)c1 << 24)) >> (8 * sh));
            uint8_t* at = row + q0;                                             // 4-byte aligned
            if (q0 >= 0 && q0 + 4 <= L) {
                *reinterpret_cast<uint32_t*>(at) = dw;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (q0 + j >= 0 && q0 + j < L) at[j] = (uint8_t)(dw >> (8 * j));
            }
        }
    }
}

static inline int64_t vis_range_bytes(int B) { return ((int64_t)B * 2 * (int64_t)sizeof(uint32_t) + 255) / 256 * 256; }

static bool extents_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    const int64_t pa = (int64_t)reinterpret_cast<intptr_t>(a), pb = (int64_t)reinterpret_cast<intptr_t>(b);
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

}  // namespace rd
using namespace rd;

extern "C" int64_t rd_render_workspace_bytes(int32_t B) {
    RD_CHECK_CODE(B >= 1 && B <= 65535, RD_EVIS_RANGE, "render_workspace_bytes: B=%d (1..65535)", B);
    return vis_range_bytes(B);
}

extern "C" int rd_render_rows(const float* rgb, int64_t rgb_stride, const float* const* planes, const int64_t* plane_strides, int32_t n_planes,
                              int32_t B, int32_t H, int32_t W, const double* range, void* workspace, const uint8_t* table, uint8_t* out,
                              int64_t frame_stride, int64_t row_pitch, void* stream) {
    RD_CHECK_CODE(planes && plane_strides && table && out && (range || workspace), RD_EVIS_NULL, "render_rows: null argument");
    RD_CHECK_CODE(B >= 1 && B <= 65535 && H >= 1 && H <= 65535 && W >= 1 && W <= 65535 && (int64_t)H * W < (1ll << 30), RD_EVIS_RANGE,
                  "render_rows: B=%d (1..65535) frame %dx%d (sides 1..65535, fewer than 2^30 pixels)", B, H, W);
    RD_CHECK_CODE(n_planes >= 1 && n_planes <= 3, RD_EVIS_PLANES, "render_rows: %d depth planes (1..3)", n_planes);
    const int n = H * W, k = n_planes + (rgb ? 1 : 0);
    VisPlanes pl = {};
    pl.count = n_planes;
    for (int i = 0; i < n_planes; ++i) {
        RD_CHECK_CODE(planes[i], RD_EVIS_NULL, "render_rows: depth plane %d is null", i);
        RD_CHECK_CODE(plane_strides[i] >= n, RD_EVIS_STRIDE, "render_rows: batch stride %lld of depth plane %d below the %d pixels of a frame",
                      (long long)plane_strides[i], i, n);
        pl.p[i] = planes[i], pl.stride[i] = plane_strides[i];
    }
    RD_CHECK_CODE(!rgb || rgb_stride >= 3 * (int64_t)n, RD_EVIS_STRIDE, "render_rows: batch stride %lld of rgb below the %lld values of a frame",
                  (long long)rgb_stride, 3ll * n);
    const int64_t L = 3ll * k * W;
    RD_CHECK_CODE(row_pitch >= L && frame_stride >= (int64_t)H * row_pitch, RD_EVIS_PITCH,
                  "render_rows: row pitch %lld below the %lld bytes of a row, or frame stride %lld below %d rows of that pitch", (long long)row_pitch,
                  (long long)L, (long long)frame_stride, H);
    RD_CHECK_CODE(!range || (range[0] == range[0] && range[1] == range[1]), RD_EVIS_NAN, "render_rows: NaN in the given range");
    const int64_t out_bytes = (int64_t)(B - 1) * frame_stride + (int64_t)(H - 1) * row_pitch + L;
    for (int i = 0; i < n_planes; ++i)
        RD_CHECK_CODE(!extents_overlap(out, out_bytes, pl.p[i], ((int64_t)(B - 1) * pl.stride[i] + n) * 4), RD_EVIS_OVERLAP,
                      "render_rows: out overlaps depth plane %d", i);
    RD_CHECK_CODE(!rgb || !extents_overlap(out, out_bytes, rgb, ((int64_t)(B - 1) * rgb_stride + 3ll * n) * 4), RD_EVIS_OVERLAP,
                  "render_rows: out overlaps rgb");
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t* rng = nullptr;
    float lo = 0.f, denom = 1.f;
    if (range) {
        // numpy: depth - d_min rounds the Python float to float32; d_max - d_min is a float64 difference, rounded when it divides
        lo = (float)range[0], denom = (float)(range[1] - range[0]);
    } else {
        rng = static_cast<uint32_t*>(workspace);
        RD_CHECK_HIP(hipMemsetAsync(rng, 0, (size_t)vis_range_bytes(B), s));
        bool vec = n % 4 == 0;
        for (int i = 0; i < n_planes; ++i) vec = vec && reinterpret_cast<uintptr_t>(pl.p[i]) % 16 == 0 && pl.stride[i] % 4 == 0;
        const int per_block = kVisBlock * (vec ? 16 : 4);                       // pixels of a plane a block reads at least
        const dim3 grid((int)std::min<int64_t>(cdiv64(n, per_block), std::max(1, num_cus() * 8 / B)), B);
        if (vec) hipLaunchKernelGGL(range_kernel<true>, grid, dim3(kVisBlock), 0, s, pl, n, rng);
        else hipLaunchKernelGGL(range_kernel<false>, grid, dim3(kVisBlock), 0, s, pl, n, rng);
        RD_CHECK_LAUNCH("range_kernel");
    }
    const dim3 grid(std::min(H, std::max(1, num_cus() * 8 / B)), B);
    hipLaunchKernelGGL(render_kernel, grid, dim3(kVisBlock), 0, s, rgb, rgb_stride, pl, H, W, rng, lo, denom, table, out, frame_stride, row_pitch);
    RD_CHECK_LAUNCH("render_kernel");
    return RD_OK;
}
