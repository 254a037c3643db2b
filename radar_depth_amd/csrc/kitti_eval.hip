// The KITTI depth devkit's evaluation on the GPU (the reference: misc/devkit/cpp/evaluate_depth.cpp, io_depth.h, log_colormap.h, utils.h):
// readDepthMap / writeDepthMap, interpolateBackground, depthError, errorImage(D_gt, true) and statMean / statMin / statMax, with the
// devkit's arithmetic and quirks.  A depth plane is float32, valid where d >= 0 (NaN fails the comparison; 0.0 and -0.0 pass).
//   kitti_rows_kernel    the row pass of interpolateBackground.  One wavefront per row, four rows per workgroup.  A left-to-right sweep
//                        in 64-pixel chunks: a 64-bit ballot of the valid lanes, the highest set bit below a lane names the lane whose
//                        value is its left candidate, one carried value crosses chunks.  The sweep writes into `out` every valid pixel
//                        as it is and, for an invalid pixel with a left candidate L, the COMPLEMENT of L's bits: a candidate is >= 0 or
//                        -0.0, so its complement is negative or NaN and still reads as invalid.  That keeps the original validity of
//                        the row readable from `out` alone, which is what lets out be `in`.  The right-to-left sweep then reads `out`,
//                        finds the right candidates the same way and writes R < L ? R : L (std::min(L, R)), L or R.  A pixel left of
//                        the row's first valid pixel has no L; the wave remembers that column.  One flag per row goes to ws.
//   kitti_cols_kernel    every workgroup finds the first and the last flagged row itself and copies rows above / below them.  Flagged
//                        rows are complete after the row pass; an unflagged row between two flagged ones is left alone (the reference
//                        only extrapolates to the top and the bottom).
//   kitti_err_*          depthError: ten float64 accumulators per thread (eight sums, sum of the signed log difference, count), the
//                        wave's lanes by wave_total_lane63, the four waves in order, partials per block, one block per frame for the
//                        final sums and the nine values.  The number of blocks depends on (H, W) only, so the bits do not depend on
//                        the device either.
//   kitti_image_kernel   errorImage with log colours as a gather (the reference splats every centre over its 3x3 neighbourhood in raster
//                        order, later writes winning): an output pixel takes the last centre in raster order, among its up to
//                        nine neighbour centres, that has a valid ground truth (kitti_pixel).  Output as in render_kernel
//                        (visualize.hip): a thread owns an aligned dword of the row, partial first / last dwords go byte by byte.
//   kitti_stats_kernel   statMean's sum, statMin, statMax and the frame count per metric, rows folded in order by one thread a metric.
// Contraction is off for the whole file and the float32 divisions are __fdiv_rn.
#include "common.h"

#include <algorithm>
#include <math.h>

#pragma clang fp contract(off)

namespace rd {

constexpr int kKittiBlock = 256;                    // four wavefronts: the LDS arrays below have four rows
constexpr int kKittiMaxBlocks = 256;                // partial blocks per frame of the error sums (one per thread of the final block)
constexpr int kKittiBins = 10;

struct KittiColormap {                              // by value in the kernel arguments
    float lo[kKittiBins], hi[kKittiBins];
    uint32_t rgb[kKittiBins];                       // R | G << 8 | B << 16
};
typedef KittiColormap KittiBinsLds;                 // the same rows in LDS, filled once per workgroup

__global__ __launch_bounds__(kKittiBlock) void kitti_decode_kernel(const uint16_t* __restrict__ in, int64_t in_stride, float* __restrict__ out,
                                                                   int64_t out_stride, int64_t n) {
    const uint16_t* src = in + (int64_t)blockIdx.y * in_stride;
    float* dst = out + (int64_t)blockIdx.y * out_stride;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const uint16_t v = src[e];
        dst[e] = v == 0 ? -1.f : (float)((double)(float)v / 256.0);
    }
}

__global__ __launch_bounds__(kKittiBlock) void kitti_encode_kernel(const float* __restrict__ in, int64_t in_stride, uint16_t* __restrict__ out,
                                                                   int64_t out_stride, int64_t n) {
    const float* src = in + (int64_t)blockIdx.y * in_stride;
    uint16_t* dst = out + (int64_t)blockIdx.y * out_stride;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const float d = src[e];
        uint16_t r = 0;
        if (d >= 0.f) {
            double v = (double)d * 256.0;
            v = v < 1.0 ? 1.0 : v;                                              // std::max(v, 1.0)
            r = v >= 65535.0 ? (uint16_t)65535 : (uint16_t)(int)v;             // (the reference's cast is undefined above 65535)
        }
        dst[e] = r;
    }
}

// in and out may be the same plane: no __restrict__
__global__ __launch_bounds__(kKittiBlock) void kitti_rows_kernel(const float* in, int64_t in_stride, float* out, int64_t out_stride, int H, int W,
                                                                 int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int y = blockIdx.x * (kKittiBlock / 64) + (threadIdx.x >> 6);
    if (y >= H) return;                                                         // whole waves; the kernel has no barrier
    const int b = blockIdx.y;
    const float* src = in + (int64_t)b * in_stride + (int64_t)y * W;
    float* dst = out + (int64_t)b * out_stride + (int64_t)y * W;
    const int chunks = (W + 63) >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    float carry = -1.f;
    bool have = false;
    int first = W;                                                              // column of the row's first valid pixel
    for (int c = 0; c < chunks; ++c) {
        const int x = c * 64 + lane;
        const float v = x < W ? src[x] : -1.f;
        const bool ok = v >= 0.f;
        const unsigned long long m = __ballot(ok);
        const unsigned long long mb = m & below;
        const float lv = __shfl(v, mb ? 63 - __clzll((long long)mb) : 0, 64);
        const float L = mb ? lv : carry;
        const bool has_l = mb != 0 || have;
        if (x < W) dst[x] = (!ok && has_l) ? __uint_as_float(~__float_as_uint(L)) : v;
        if (m) {                                                                // uniform
            if (!have) first = c * 64 + __ffsll(m) - 1;
            carry = __shfl(v, 63 - __clzll((long long)m), 64);
            have = true;
        }
    }
    if (lane == 0) flags[(int64_t)b * H + y] = have ? 1 : 0;
    if (!have) return;                                                          // uniform: the row keeps its values
    // the lanes read below what other lanes of this wave wrote above: the stores have to be complete, and a CU's waves share its L1,
    // so workgroup scope is enough (an agent-scope fence per row would write back the L2: microseconds each)
    __threadfence_block();
    bool have_r = false;
    carry = -1.f;
    for (int c = chunks - 1; c >= 0; --c) {
        const int x = c * 64 + lane;
        const float v = x < W ? dst[x] : -1.f;
        const bool ok = v >= 0.f;
        const unsigned long long m = __ballot(ok);
        const unsigned long long ma = m & ~((2ull << lane) - 1ull);            // lanes above this one (lane 63: 2 << 63 == 0, none)
        const float rv = __shfl(v, ma ? __ffsll(ma) - 1 : 0, 64);
        const float R = ma ? rv : carry;
        const bool has_r = ma != 0 || have_r;
        if (x < W && !ok) {
            const float L = __uint_as_float(~__float_as_uint(v));               // meaningful only right of `first`
            dst[x] = x > first ? (has_r ? (R < L ? R : L) : L) : R;
        }
        if (m) {                                                                // uniform
            carry = __shfl(v, __ffsll(m) - 1, 64);
            have_r = true;
        }
    }
}

__global__ __launch_bounds__(kKittiBlock) void kitti_cols_kernel(float* __restrict__ out, int64_t out_stride, int H, int W,
                                                                 const int32_t* __restrict__ flags) {
    __shared__ int part[2][kKittiBlock / 64];
    static_assert(kKittiBlock == 256, "the reduction below reads four partial values");
    const int b = blockIdx.y;
    const int32_t* f = flags + (int64_t)b * H;
    int lo = H, hi = -1;
    for (int y = threadIdx.x; y < H; y += blockDim.x)
        if (f[y]) lo = min(lo, y), hi = max(hi, y);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o, 64)), hi = max(hi, __shfl_xor(hi, o, 64));
    if ((threadIdx.x & 63) == 0) part[0][threadIdx.x >> 6] = lo, part[1][threadIdx.x >> 6] = hi;
    rd_sync();                                                                  // reached by every thread of the block
    lo = min(min(part[0][0], part[0][1]), min(part[0][2], part[0][3]));
    hi = max(max(part[1][0], part[1][1]), max(part[1][2], part[1][3]));
    if (hi < 0) return;                                                         // a frame without a valid pixel
    float* base = out + (int64_t)b * out_stride;
    const int outer = lo + (H - 1 - hi);                                        // rows above the first and below the last valid row
    for (int k = blockIdx.x; k < outer; k += gridDim.x) {
        const int y = k < lo ? k : hi + 1 + (k - lo);
        const float* src = base + (int64_t)(k < lo ? lo : hi) * W;
        float* dst = base + (int64_t)y * W;
        for (int x = threadIdx.x; x < W; x += blockDim.x) dst[x] = src[x];
    }
}

// the ten per-pixel terms of depthError, each in the reference's type, added into float64 accumulators
__device__ __forceinline__ void kitti_terms(float gt, float p, double* acc) {
    const float d = fabsf(gt - p);
    const float d2 = d * d;
    const float di = (float)fabs(1.0 / (double)gt - 1.0 / (double)p);
    const float di2 = di * di;
    const double ld = log((double)gt) - log((double)p);
    const float dl = (float)fabs(ld);
    const float dl2 = dl * dl;
    const float rel = __fdiv_rn(d, gt);
    const float sq = __fdiv_rn(d2, gt * gt);
    acc[0] += (double)d;
    acc[1] += (double)d2;
    acc[2] += (double)di;
    acc[3] += (double)di2;
    acc[4] += (double)dl;
    acc[5] += (double)dl2;
    acc[6] += ld;
    acc[7] += (double)rel;
    acc[8] += (double)sq;
    acc[9] += 1.0;
}

// ten sums over the block (all lanes active): the lanes' fixed tree, then the four waves in order; valid in threads 0..9 (thread i: sum i)
__device__ __forceinline__ double kitti_block_sums(const double* acc, double (*sh)[10]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const double v = wave_total_lane63(acc[i]);
        if ((threadIdx.x & 63) == 63) sh[threadIdx.x >> 6][i] = v;
    }
    rd_sync();                                                                  // reached by every thread of the block
    const int i = threadIdx.x < 10 ? threadIdx.x : 0;
    return ((sh[0][i] + sh[1][i]) + sh[2][i]) + sh[3][i];
}

__global__ __launch_bounds__(kKittiBlock) void kitti_err_partial_kernel(const float* __restrict__ gt, int64_t gt_stride,
                                                                        const float* __restrict__ pred, int64_t pred_stride, int64_t n,
                                                                        int zero_invalid, double* __restrict__ part) {
    __shared__ double sh[kKittiBlock / 64][10];
    const float* g = gt + (int64_t)blockIdx.y * gt_stride;
    const float* p = pred + (int64_t)blockIdx.y * pred_stride;
    double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const float t = g[e];
        if (zero_invalid ? t > 0.f : t >= 0.f) kitti_terms(t, p[e], acc);
    }
    const double s = kitti_block_sums(acc, sh);
    if (threadIdx.x < 10) part[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 10 + threadIdx.x] = s;
}

__global__ __launch_bounds__(kKittiBlock) void kitti_err_final_kernel(const double* __restrict__ part, int nb, double* __restrict__ out) {
    __shared__ double sh[kKittiBlock / 64][10];
    __shared__ double tot[10];
    double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if ((int)threadIdx.x < nb) {                                                // nb <= kKittiBlock
        const double* row = part + ((int64_t)blockIdx.x * nb + threadIdx.x) * 10;
#pragma unroll
        for (int i = 0; i < 10; ++i) acc[i] = row[i];
    }
    const double s = kitti_block_sums(acc, sh);
    if (threadIdx.x < 10) tot[threadIdx.x] = s;
    rd_sync();                                                                  // reached by every thread of the block
    if (threadIdx.x >= 10) return;
    const double n = tot[9];
    double v;
    switch (threadIdx.x) {
        case 0: v = tot[0] / n; break;
        case 1: v = sqrt(tot[1] / n); break;
        case 2: v = tot[2] / n; break;
        case 3: v = sqrt(tot[3] / n); break;
        case 4: v = tot[4] / n; break;
        case 5: v = sqrt(tot[5] / n); break;
        case 6: {
            const double mean = tot[6] / n;
            v = sqrt(tot[5] / n - mean * mean);
            break;
        }
        case 7: v = tot[7] / n; break;
        case 8: v = tot[8] / n; break;
        default: v = n; break;
    }
    out[(int64_t)blockIdx.x * 10 + threadIdx.x] = v;
}

// colour of a centre with ground truth t and prediction q: R | G << 8 | B << 16
__device__ __forceinline__ uint32_t kitti_colour(float t, float q, const KittiBinsLds& cm) {
    const float d_err = fabsf(q - t), d_mag = fabsf(t);
    const double a = (double)d_err / 3.0, b = 20.0 * (double)d_err / (double)d_mag;
    const float n_err = (float)(b < a ? b : a);                                 // std::min(a, b), kept in a float as in the reference
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < kKittiBins; ++i)
        if (n_err >= cm.lo[i] && n_err < cm.hi[i]) c = cm.rgb[i];
    return c;
}

__device__ __forceinline__ bool kitti_is_centre(int v, int u, int H, int W) { return v >= 1 && v <= H - 2 && u >= 1 && u <= W - 2; }

// pixel m of row y (0 <= m < W; anything else gives 0 and reads nothing): the last qualifying centre among the 3x3 neighbours.  The last
// centre in raster order is tried first: with a dense ground truth it wins and nothing else is read.  Otherwise the other eight
// ground-truth loads are issued together, none depending on another (measured on sixteen 450x800 frames: a backwards search that stops
// at the first hit waits for every load before it issues the next, 179 us with 0.8 % valid; nine unconditional loads, 100 us whatever
// the density); the prediction is read at the one centre that wins.
__device__ __forceinline__ uint32_t kitti_pixel(int m, int y, int H, int W, const float* __restrict__ g, const float* __restrict__ p,
                                                int zero_invalid, const KittiBinsLds& cm) {
    if (m < 0 || m >= W) return 0u;
    if (kitti_is_centre(y + 1, m + 1, H, W)) {
        const int64_t at = (int64_t)(y + 1) * W + (m + 1);
        const float t = g[at];
        if (zero_invalid ? t > 0.f : t >= 0.f) return kitti_colour(t, p[at], cm);
    }
    int64_t best = -1;
    float tb = 0.f;
#pragma unroll
    for (int dv = -1; dv <= 1; ++dv)
#pragma unroll
        for (int du = -1; du <= 1; ++du) {                                      // raster order of the centres: a later one replaces
            if (dv == 1 && du == 1) continue;
            const bool in = kitti_is_centre(y + dv, m + du, H, W);
            const int64_t at = (int64_t)(y + dv) * W + (m + du);
            const float t = in ? g[at] : -1.f;
            if (in && (zero_invalid ? t > 0.f : t >= 0.f)) best = at, tb = t;
        }
    return best < 0 ? 0u : kitti_colour(tb, p[best], cm);
}

__global__ __launch_bounds__(kKittiBlock) void kitti_image_kernel(const float* __restrict__ gt, int64_t gt_stride, const float* __restrict__ pred,
                                                                  int64_t pred_stride, int H, int W, int zero_invalid,
                                                                  const KittiColormap table, uint8_t* __restrict__ out, int64_t frame_stride,
                                                                  int64_t row_pitch) {
    __shared__ KittiBinsLds cm;                                                 // (thirty words held in scalar registers crowded them out)
    if (threadIdx.x < kKittiBins) {
        cm.lo[threadIdx.x] = table.lo[threadIdx.x];
        cm.hi[threadIdx.x] = table.hi[threadIdx.x];
        cm.rgb[threadIdx.x] = table.rgb[threadIdx.x];
    }
    rd_sync();                                                                  // reached by every thread of the block
    const int b = blockIdx.y;
    const float* g = gt + (int64_t)b * gt_stride;
    const float* p = pred + (int64_t)b * pred_stride;
    const int L = 3 * W;                                                        // bytes of an output row
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        uint8_t* row = out + (int64_t)b * frame_stride + (int64_t)y * row_pitch;
        const int a0 = (int)(reinterpret_cast<uintptr_t>(row) & 3);            // the row starts a0 bytes into its first dword
        const int ndw = (a0 + L + 3) >> 2;
        for (int i = threadIdx.x; i < ndw; i += blockDim.x) {
            const int q0 = 4 * i - a0;                                          // row byte of this dword's byte 0: -3 .. L-1
            const int m0 = (q0 + 3) / 3 - 1, sh = (q0 + 3) - 3 * (m0 + 1);     // q0 = 3 * m0 + sh, m0 >= -1
            const uint32_t c0 = kitti_pixel(m0, y, H, W, g, p, zero_invalid, cm);
            const uint32_t c1 = kitti_pixel(m0 + 1, y, H, W, g, p, zero_invalid, cm);
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

// state[9][4]: sum, minimum, maximum, frames.  One thread a metric walks the rows in order.
__global__ __launch_bounds__(64) void kitti_stats_kernel(const double* __restrict__ errors, int rows, double* __restrict__ state) {
    if (threadIdx.x >= 9) return;
    double* s = state + 4 * threadIdx.x;
    double sum = s[0], mn = s[1], mx = s[2], cnt = s[3];
    for (int r = 0; r < rows; ++r) {
        const double e = errors[(int64_t)r * 10 + threadIdx.x];
        sum += e;
        if (e < mn) mn = e;
        if (e > mx) mx = e;
        cnt += 1.0;
    }
    s[0] = sum, s[1] = mn, s[2] = mx, s[3] = cnt;
}

static inline bool kitti_dims_ok(int B, int H, int W) { return B >= 1 && B <= 65535 && H >= 1 && H <= 65535 && W >= 1 && W <= 65535; }
static inline int kitti_err_blocks(int64_t n) { return (int)std::min<int64_t>(cdiv64(n, 4 * kKittiBlock), kKittiMaxBlocks); }
static inline bool aligned8(const void* p) { return reinterpret_cast<uintptr_t>(p) % 8 == 0; }

}  // namespace rd
using namespace rd;

#define RD_KITTI_DIMS(who_)                                                                                                    \
    RD_CHECK_CODE(kitti_dims_ok(B, H, W), RD_EKITTI_RANGE, "%s: B=%d frame %dx%d (each 1..65535)", who_, B, H, W)
#define RD_KITTI_STRIDE(who_, what_, s_)                                                                                       \
    RD_CHECK_CODE((s_) >= (int64_t)H * W, RD_EKITTI_STRIDE, "%s: frame stride %lld of %s below the %lld pixels of a frame", who_, \
                  (long long)(s_), what_, (long long)H * W)

extern "C" int64_t rd_kitti_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    RD_KITTI_DIMS("kitti_workspace_bytes");
    const int64_t flags = (int64_t)B * H * (int64_t)sizeof(int32_t);
    const int64_t part = (int64_t)B * kitti_err_blocks((int64_t)H * W) * 10 * (int64_t)sizeof(double);
    return (std::max(flags, part) + 255) / 256 * 256;
}

extern "C" int rd_kitti_decode(const uint16_t* in, int64_t in_stride, float* out, int64_t out_stride, int32_t B, int32_t H, int32_t W,
                               void* stream) {
    RD_CHECK_CODE(in && out, RD_EKITTI_NULL, "kitti_decode: null argument");
    RD_KITTI_DIMS("kitti_decode");
    RD_KITTI_STRIDE("kitti_decode", "in", in_stride);
    RD_KITTI_STRIDE("kitti_decode", "out", out_stride);
    const int64_t n = (int64_t)H * W;
    const dim3 grid((int)std::min<int64_t>(cdiv64(n, 4 * kKittiBlock), 1024), B);
    hipLaunchKernelGGL(kitti_decode_kernel, grid, dim3(kKittiBlock), 0, static_cast<hipStream_t>(stream), in, in_stride, out, out_stride, n);
    RD_CHECK_LAUNCH("kitti_decode_kernel");
    return RD_OK;
}

extern "C" int rd_kitti_encode(const float* in, int64_t in_stride, uint16_t* out, int64_t out_stride, int32_t B, int32_t H, int32_t W,
                               void* stream) {
    RD_CHECK_CODE(in && out, RD_EKITTI_NULL, "kitti_encode: null argument");
    RD_KITTI_DIMS("kitti_encode");
    RD_KITTI_STRIDE("kitti_encode", "in", in_stride);
    RD_KITTI_STRIDE("kitti_encode", "out", out_stride);
    const int64_t n = (int64_t)H * W;
    const dim3 grid((int)std::min<int64_t>(cdiv64(n, 4 * kKittiBlock), 1024), B);
    hipLaunchKernelGGL(kitti_encode_kernel, grid, dim3(kKittiBlock), 0, static_cast<hipStream_t>(stream), in, in_stride, out, out_stride, n);
    RD_CHECK_LAUNCH("kitti_encode_kernel");
    return RD_OK;
}

extern "C" int rd_kitti_interpolate(const float* in, int64_t in_stride, float* out, int64_t out_stride, int32_t B, int32_t H, int32_t W,
                                    void* ws, void* stream) {
    RD_CHECK_CODE(in && out && ws, RD_EKITTI_NULL, "kitti_interpolate: null argument");
    RD_KITTI_DIMS("kitti_interpolate");
    RD_KITTI_STRIDE("kitti_interpolate", "in", in_stride);
    RD_KITTI_STRIDE("kitti_interpolate", "out", out_stride);
    RD_CHECK_CODE(aligned8(ws), RD_EKITTI_ALIGN, "kitti_interpolate: ws not 8-byte aligned");
    if (!(in == out && in_stride == out_stride)) {
        const int64_t n = (int64_t)H * W;
        const int64_t a = (int64_t)reinterpret_cast<intptr_t>(in), a_bytes = ((int64_t)(B - 1) * in_stride + n) * 4;
        const int64_t o = (int64_t)reinterpret_cast<intptr_t>(out), o_bytes = ((int64_t)(B - 1) * out_stride + n) * 4;
        RD_CHECK_CODE(!(a < o + o_bytes && o < a + a_bytes), RD_EKITTI_OVERLAP,
                      "kitti_interpolate: out overlaps in without being in (same pointer, same stride)");
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t* flags = static_cast<int32_t*>(ws);
    hipLaunchKernelGGL(kitti_rows_kernel, dim3(cdiv(H, kKittiBlock / 64), B), dim3(kKittiBlock), 0, s, in, in_stride, out, out_stride, H, W, flags);
    RD_CHECK_LAUNCH("kitti_rows_kernel");
    hipLaunchKernelGGL(kitti_cols_kernel, dim3(std::min(H, 128), B), dim3(kKittiBlock), 0, s, out, out_stride, H, W, flags);
    RD_CHECK_LAUNCH("kitti_cols_kernel");
    return RD_OK;
}

extern "C" int rd_kitti_errors(const float* gt, int64_t gt_stride, const float* pred, int64_t pred_stride, int32_t B, int32_t H, int32_t W,
                               int32_t zero_invalid, void* ws, double* out, void* stream) {
    RD_CHECK_CODE(gt && pred && ws && out, RD_EKITTI_NULL, "kitti_errors: null argument");
    RD_KITTI_DIMS("kitti_errors");
    RD_KITTI_STRIDE("kitti_errors", "gt", gt_stride);
    RD_KITTI_STRIDE("kitti_errors", "pred", pred_stride);
    RD_CHECK_CODE(aligned8(ws) && aligned8(out), RD_EKITTI_ALIGN, "kitti_errors: ws or out not 8-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n = (int64_t)H * W;
    const int nb = kitti_err_blocks(n);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(kitti_err_partial_kernel, dim3(nb, B), dim3(kKittiBlock), 0, s, gt, gt_stride, pred, pred_stride, n, zero_invalid, part);
    RD_CHECK_LAUNCH("kitti_err_partial_kernel");
    hipLaunchKernelGGL(kitti_err_final_kernel, dim3(B), dim3(kKittiBlock), 0, s, part, nb, out);
    RD_CHECK_LAUNCH("kitti_err_final_kernel");
    return RD_OK;
}

extern "C" int rd_kitti_error_image(const float* gt, int64_t gt_stride, const float* pred, int64_t pred_stride, int32_t B, int32_t H, int32_t W,
                                    int32_t zero_invalid, const float* table, uint8_t* out, int64_t frame_stride, int64_t row_pitch,
                                    void* stream) {
    RD_CHECK_CODE(gt && pred && table && out, RD_EKITTI_NULL, "kitti_error_image: null argument");
    RD_KITTI_DIMS("kitti_error_image");
    RD_KITTI_STRIDE("kitti_error_image", "gt", gt_stride);
    RD_KITTI_STRIDE("kitti_error_image", "pred", pred_stride);
    RD_CHECK_CODE(row_pitch >= 3ll * W && frame_stride >= (int64_t)H * row_pitch, RD_EKITTI_PITCH,
                  "kitti_error_image: row pitch %lld below the %lld bytes of a row, or frame stride %lld below %d rows of that pitch",
                  (long long)row_pitch, 3ll * W, (long long)frame_stride, H);
    KittiColormap cm;
    for (int i = 0; i < kKittiBins; ++i) {
        const float* r = table + 5 * i;
        cm.lo[i] = r[0], cm.hi[i] = r[1];
        cm.rgb[i] = (uint32_t)(uint8_t)r[2] | ((uint32_t)(uint8_t)r[3] << 8) | ((uint32_t)(uint8_t)r[4] << 16);
    }
    const dim3 grid(std::min(H, std::max(1, 4096 / B)), B);
    hipLaunchKernelGGL(kitti_image_kernel, grid, dim3(kKittiBlock), 0, static_cast<hipStream_t>(stream), gt, gt_stride, pred, pred_stride, H, W,
                       zero_invalid, cm, out, frame_stride, row_pitch);
    RD_CHECK_LAUNCH("kitti_image_kernel");
    return RD_OK;
}

extern "C" int rd_kitti_stats_update(const double* errors, int32_t B, double* state, void* stream) {
    RD_CHECK_CODE(errors && state, RD_EKITTI_NULL, "kitti_stats_update: null argument");
    RD_CHECK_CODE(B >= 1 && B <= 65535, RD_EKITTI_RANGE, "kitti_stats_update: B=%d (1..65535)", B);
    RD_CHECK_CODE(aligned8(errors) && aligned8(state), RD_EKITTI_ALIGN, "kitti_stats_update: errors or state not 8-byte aligned");
    hipLaunchKernelGGL(kitti_stats_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), errors, B, state);
    RD_CHECK_LAUNCH("kitti_stats_kernel");
    return RD_OK;
}
