// Distance-interval metrics: Result_multidist.evaluate and AverageMeter_multidist.update (evaluation/metrics.py:61-176) on the device.
// The reference makes one pass per interval (boolean-mask gathers, a `torch.sum(mask) == 0` synchronisation and a dozen blocking float()
// conversions each); here output and target are read once, the ten fp32 terms of a valid pixel are evaluated once (metric_terms) and
// added in fp64 into every interval the pixel is in.
#include "common.h"
#include "metric_terms.h"

#include <cmath>

namespace rd {

constexpr int MD_MAX = RD_MDIST_MAX_INTERVALS;
constexpr int MD_PIX = 4;                       // pixels per thread and trip
constexpr int MD_CHUNK = 256 * MD_PIX;          // pixels per block and trip
constexpr int MD_BLOCKS = 1024;                 // blocks per frame at most

struct MdBounds {
    float lo[MD_MAX], hi[MD_MAX];               // interval k = [lo[k], hi[k]], both closed; hi[n-1] = +inf
};

// (wave_total_lane63, the fixed-order sum of a double over a wave on the DPP path: common.h)
// A hundred fp64 accumulators per thread (ten terms x ten intervals) would live in scratch.  Instead a thread keeps the ten fp32
// terms of its MD_PIX pixels and a bitmask of the intervals each is in; the wave then visits the intervals any of its lanes holds
// (a ballot: a depth map is smooth, most waves see one or two), adds each lane's terms of that interval in fp64, reduces the ten
// sums across the lanes in a fixed order (wave_total_lane63), and lane 63 adds them into the wave's own [n][10] block of LDS.  The order
// of every addition is fixed by the geometry: trips in order, pixels in order, the lanes' tree, the waves of a block in order, the
// blocks in md_final_kernel's order.
// VEC: frames and rows are 16-byte aligned (hw % 4 == 0, aligned bases) -- one float4 of each tensor per thread and trip.
template <bool VEC>
__global__ __launch_bounds__(256) void md_partial_kernel(const float* __restrict__ out, const float* __restrict__ target, int64_t hw,
                                                         int n, MdBounds b, double* __restrict__ part) {
    __shared__ double acc[4][MD_MAX * 10];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int i = lane; i < n * 10; i += 64) acc[w][i] = 0.0;          // (a wave touches its own block only: no barrier until the end)
    const float* o = out + (size_t)blockIdx.y * hw;
    const float* tg = target + (size_t)blockIdx.y * hw;
    for (int64_t base = (int64_t)blockIdx.x * MD_CHUNK; base < hw; base += (int64_t)gridDim.x * MD_CHUNK) {
        float ov[MD_PIX], tv[MD_PIX];
        if (VEC) {
            const int64_t e = base + (int64_t)threadIdx.x * MD_PIX;
            float4 a = make_float4(1.f, 1.f, 1.f, 1.f), t4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < hw) {                                               // (hw % 4 == 0: a quad is inside or outside as a whole)
                a = ld4(o + e);
                t4 = ld4(tg + e);
            }
            ov[0] = a.x; ov[1] = a.y; ov[2] = a.z; ov[3] = a.w;
            tv[0] = t4.x; tv[1] = t4.y; tv[2] = t4.z; tv[3] = t4.w;
        } else {
#pragma unroll
            for (int p = 0; p < MD_PIX; ++p) {
                const int64_t e = base + p * 256 + threadIdx.x;
                const bool in = e < hw;
                ov[p] = in ? o[e] : 1.f;
                tv[p] = in ? tg[e] : 0.f;
            }
        }
        float tm[MD_PIX][10];
        unsigned member[MD_PIX], any = 0;
#pragma unroll
        for (int p = 0; p < MD_PIX; ++p) {
            const float t = tv[p];
            unsigned m = 0;
            if (t > 0.f) {
#pragma unroll
                for (int k = 0; k < MD_MAX; ++k)
                    if (k < n && t >= b.lo[k] && t <= b.hi[k]) m |= 1u << k;
            }
            member[p] = m;
            any |= m;
            double one[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            metric_terms(ov[p], t, one);                                // (0 + an fp32 term: the term itself, exactly)
#pragma unroll
            for (int i = 0; i < 10; ++i) tm[p][i] = (float)one[i];
        }
        for (int k = 0; k < n; ++k) {
            if (__ballot((any >> k) & 1u) == 0ull) continue;           // wave-uniform
            double s[10];
#pragma unroll
            for (int i = 0; i < 10; ++i) s[i] = 0.0;
#pragma unroll
            for (int p = 0; p < MD_PIX; ++p) {
                const bool in = (member[p] >> k) & 1u;
#pragma unroll
                for (int i = 0; i < 10; ++i) s[i] += in ? (double)tm[p][i] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                const double v = wave_total_lane63(s[i]);
                if (lane == 63) acc[w][k * 10 + i] += v;
            }
        }
    }
    rd_sync();
    double* dst = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(n * 10);
    for (int i = threadIdx.x; i < n * 10; i += blockDim.x) dst[i] = ((acc[0][i] + acc[1][i]) + acc[2][i]) + acc[3][i];
}

// sums[frame][k][10] = the blocks' partial sums of that frame and interval: one workgroup each (grid (n, frames)).  Thread (g, j),
// g < 25, j < 10, adds word j of the blocks g, g + 25, ... in that order -- ten neighbouring threads read ten neighbouring doubles,
// and the loads of a thread do not wait for one another -- and the first ten threads add the 25 partial sums in order.  (One wave
// per word walking up to 1024 blocks one dependent load at a time took 160 us of a 195 us call at b = 16, 450x800.)
constexpr int MD_FIN_GROUPS = 25;
__global__ __launch_bounds__(256) void md_final_kernel(const double* __restrict__ part, int nb, int n, double* __restrict__ sums) {
    __shared__ double sh[MD_FIN_GROUPS][10];
    const int k = blockIdx.x, g = threadIdx.x / 10, j = threadIdx.x - g * 10;
    const int words = n * 10;
    const double* p = part + (size_t)blockIdx.y * nb * words + k * 10 + j;
    if (g < MD_FIN_GROUPS) {
        double s = 0.0;
#pragma unroll 8
        for (int i = g; i < nb; i += MD_FIN_GROUPS) s += p[(size_t)i * words];
        sh[g][j] = s;
    }
    rd_sync();
    if (threadIdx.x < 10) {
        double s = 0.0;
        for (int i = 0; i < MD_FIN_GROUPS; ++i) s += sh[i][threadIdx.x];
        sums[((size_t)blockIdx.y * n + k) * 10 + threadIdx.x] = s;
    }
}

// rd_meter_update's kernel per interval: thread (g, k, j) owns word j of meter[g][k] and walks the rows in order; a row whose
// interval k is empty (count 0) is skipped as a whole -- AverageMeter_multidist.update passes over valid_label == 0
__global__ __launch_bounds__(256) void md_meter_update_kernel(const double* __restrict__ sums, int rows, int n, const double* __restrict__ weights,
                                                              const int32_t* __restrict__ groups, int n_groups, double* __restrict__ meter,
                                                              double* __restrict__ last, int32_t* __restrict__ valid) {
    for (int i = threadIdx.x; i < n_groups * n * 12; i += blockDim.x) {
        const int g = i / (n * 12), k = (i - g * n * 12) / 12, j = i % 12;
        double v = meter[i];
        for (int r = 0; r < rows; ++r) {
            const int32_t mask = groups ? groups[r] : 1;
            const double* row = sums + ((size_t)r * n + k) * 10;
            if (!((mask >> g) & 1) || !(row[0] > 0.0)) continue;
            const double wt = weights ? weights[r] : 1.0;
            if (j == 0) v += wt;
            else if (j == 11) v += 1.0;
            else v += wt * meter_metric(row, j - 1);
        }
        meter[i] = v;
    }
    for (int i = threadIdx.x; i < n * 10; i += blockDim.x) {
        const double* row = sums + ((size_t)(rows - 1) * n + i / 10) * 10;
        last[i] = row[0] > 0.0 ? meter_metric(row, i % 10) : (double)NAN;
    }
    for (int k = threadIdx.x; k < n; k += blockDim.x) valid[k] = sums[((size_t)(rows - 1) * n + k) * 10] > 0.0 ? 1 : 0;
}

static int md_grid(int64_t hw) {
    int64_t g = cdiv64(hw, 2 * MD_CHUNK);
    if (g > MD_BLOCKS) g = MD_BLOCKS;
    return (int)(g < 1 ? 1 : g);
}

static const float MD_REFERENCE_EDGES[10] = {10.f, 20.f, 30.f, 40.f, 50.f, 60.f, 70.f, 80.f, 90.f, 100.f};

static int md_check_geometry(const char* what, int32_t frames, int64_t hw, int32_t n) {
    RD_CHECK_CODE(frames >= 1 && hw >= 1, RD_EMDIST_RANGE, "%s: frames = %d, hw = %lld: at least one frame of one pixel is needed", what, frames,
                  (long long)hw);
    RD_CHECK_CODE(n >= 1 && n <= MD_MAX, RD_EMDIST_RANGE, "%s: n_intervals = %d, 1..%d are served", what, n, MD_MAX);
    RD_CHECK_CODE(frames <= 65535, RD_EMDIST_FRAMES, "%s: at most 65535 frames per call, got %d", what, frames);
    return RD_OK;
}

}  // namespace rd
using namespace rd;

extern "C" int64_t rd_depth_metrics_multidist_workspace_floats(int32_t frames, int64_t hw, int32_t n_intervals) {
    const int rc = md_check_geometry("depth_metrics_multidist_workspace_floats", frames, hw, n_intervals);
    if (rc != RD_OK) return rc;
    return 2 * (int64_t)frames * md_grid(hw) * n_intervals * 10;
}

extern "C" int rd_depth_metrics_multidist(const float* output, const float* target, int32_t frames, int64_t hw, const float* edges,
                                          int32_t n_intervals, float* ws, double* sums, void* stream) {
    const char* what = "depth_metrics_multidist";
    RD_CHECK_CODE(output && target && ws && sums, RD_EMDIST_NULL, "%s: null argument", what);
    const int rc = md_check_geometry(what, frames, hw, n_intervals);
    if (rc != RD_OK) return rc;
    RD_CHECK_CODE(edges || n_intervals == 10, RD_EMDIST_RANGE, "%s: the default edges are ten intervals, n_intervals = %d needs its own", what,
                  n_intervals);
    RD_CHECK_CODE((((uintptr_t)ws | (uintptr_t)sums) & 7) == 0, RD_EMDIST_ALIGN, "%s: the workspace and the sums have to be 8-byte aligned", what);
    if (!edges) edges = MD_REFERENCE_EDGES;
    MdBounds b;
    for (int k = 0; k < MD_MAX; ++k) {
        b.lo[k] = INFINITY;                     // (unused slots hold no pixel)
        b.hi[k] = -INFINITY;
    }
    for (int k = 0; k < n_intervals; ++k) {
        RD_CHECK_CODE(std::isfinite(edges[k]) && edges[k] > 0.f && (k == 0 || edges[k] > edges[k - 1]), RD_EMDIST_EDGES,
                      "%s: edges[%d] = %g: the edges have to be finite, positive and strictly increasing", what, k, (double)edges[k]);
        b.lo[k] = k == 0 ? 0.f : edges[k - 1];
        b.hi[k] = k == n_intervals - 1 ? INFINITY : edges[k];
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int g = md_grid(hw);
    double* part = reinterpret_cast<double*>(ws);
    const bool vec = hw % 4 == 0 && aligned16(output) && aligned16(target);
    if (vec) hipLaunchKernelGGL(md_partial_kernel<true>, dim3(g, frames), dim3(256), 0, s, output, target, hw, n_intervals, b, part);
    else hipLaunchKernelGGL(md_partial_kernel<false>, dim3(g, frames), dim3(256), 0, s, output, target, hw, n_intervals, b, part);
    RD_CHECK_LAUNCH("md_partial_kernel");
    hipLaunchKernelGGL(md_final_kernel, dim3(n_intervals, frames), dim3(256), 0, s, part, g, n_intervals, sums);
    RD_CHECK_LAUNCH("md_final_kernel");
    return RD_OK;
}

extern "C" int rd_meter_update_multidist(const double* sums, int32_t rows, int32_t n_intervals, const double* weights, const int32_t* groups,
                                         int32_t n_groups, double* meter, double* last, int32_t* valid, void* stream) {
    const char* what = "meter_update_multidist";
    RD_CHECK_CODE(sums && meter && last && valid, RD_EMDIST_NULL, "%s: null argument", what);
    RD_CHECK_CODE(rows >= 1, RD_EMDIST_RANGE, "%s: rows = %d, at least one is needed", what, rows);
    RD_CHECK_CODE(n_intervals >= 1 && n_intervals <= MD_MAX, RD_EMDIST_RANGE, "%s: n_intervals = %d, 1..%d are served", what, n_intervals, MD_MAX);
    RD_CHECK_CODE(n_groups >= 1 && n_groups <= 31, RD_EMDIST_RANGE, "%s: n_groups must be 1..31 (one bit of an int32 mask each), got %d", what,
                  n_groups);
    RD_CHECK_CODE((((uintptr_t)sums | (uintptr_t)meter | (uintptr_t)last) & 7) == 0 && ((uintptr_t)valid & 3) == 0, RD_EMDIST_ALIGN,
                  "%s: sums, meter and last have to be 8-byte aligned, valid 4-byte aligned", what);
    hipLaunchKernelGGL(md_meter_update_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), sums, rows, n_intervals, weights, groups,
                       n_groups, meter, last, valid);
    RD_CHECK_LAUNCH("md_meter_update_kernel");
    return RD_OK;
}
