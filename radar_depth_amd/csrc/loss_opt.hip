// Losses, the multistage radar filter and the optimizer step -- the tail of the reference's training-step body
// (main.py:416-445): MaskedL1Loss (evaluation/criteria_new.py:44-54), MaskedBerHuLoss (:57-81), SmoothnessLoss (:8-28), the
// uncertainty-weighted total (main.py:423-429), Filter_layer (model/multistage_model.py:87-119) and
// torch.optim.SGD with momentum + weight decay (main.py:285-290,445).  All scalars stay on the device.
#include "metric_terms.h"
#include "step_tail.h"

namespace rd {

__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = wave_sum_d(v);
    const int w = threadIdx.x >> 6;
    rd_sync();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    rd_sync();
    double s = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) s += sh[i];
    return s;
}

// ---------------------------------------------------------------- masked L1 / L2
// SQ = false: MaskedL1Loss (sum |t-p|); SQ = true: MaskedMSELoss (criteria_new.py:31-41, sum (t-p)^2)
template <bool SQ>
__global__ __launch_bounds__(256) void l1_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, int64_t n,
                                                     const double* __restrict__ sums, const float* __restrict__ coef,
                                                     float* __restrict__ dpred, int accumulate) {
    const float k = (float)((double)coef[0] / sums[1]);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const float t = target[e];
        float g = 0.f;
        if (t > 0.f) {
            const float diff = t - pred[e];
            g = SQ ? -2.f * diff * k : (diff > 0.f ? -k : (diff < 0.f ? k : 0.f));
        }
        dpred[e] = accumulate ? dpred[e] + g : g;
    }
}

// ---------------------------------------------------------------- masked BerHu (criteria_new.py:57-81)
// The reference forms delta = thresh * max|t-p| on the host (a blocking .item() in the middle of the loss) and then works in fp32
// tensors with delta, delta^2 and 2 delta rounded to fp32 where they meet one.  Here the maximum stays on the device: pass 1 leaves one
// maximum per block, every block of pass 2 reduces those (<= RED_BLOCKS words) and forms the three constants itself.
// The maximum is taken on the BITS of |t-p|: non-negative floats order as unsigned integers, so it is exact and independent of the
// order, and a NaN difference (a diverged prediction) is the largest of all and reaches the loss as it does in the reference.
__device__ __forceinline__ unsigned block_max_u(unsigned v, unsigned* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned w = (unsigned)__shfl_xor((int)v, o, 64);
        v = w > v ? w : v;
    }
    rd_sync();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    rd_sync();
    unsigned m = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) m = sh[i] > m ? sh[i] : m;
    return m;
}
__device__ __forceinline__ unsigned blocks_max_u(const unsigned* __restrict__ pmax, int nblocks, unsigned* sh) {
    unsigned m = 0;
    for (int i = threadIdx.x; i < nblocks; i += blockDim.x) m = pmax[i] > m ? pmax[i] : m;
    return block_max_u(m, sh);
}

struct BerhuConsts { float thr, d2, den; };
__device__ __forceinline__ BerhuConsts berhu_consts(double delta) {
    BerhuConsts k;
    k.thr = (float)(-delta);
    k.d2 = (float)(delta * delta);
    k.den = (float)(2.0 * delta);
    return k;
}
// The two branch decisions of one valid pixel: separate fp32 comparisons (a pixel can fail both), every operation rounded on its own.
__device__ __forceinline__ float berhu_branches(float diff, const BerhuConsts& k, bool& in1, bool& in2) {
#pragma clang fp contract(off)
    const float y = diff * diff - k.d2;
    in1 = -diff > k.thr;
    in2 = y > 0.f;
    return y;
}
__device__ __forceinline__ float berhu_term(float diff, const BerhuConsts& k) {
#pragma clang fp contract(off)
    bool in1, in2;
    const float y = berhu_branches(diff, k, in1, in2);
    const float part1 = in1 ? diff : 0.f;
    const float part2 = __fdiv_rn((in2 ? y : -k.d2) + k.d2, k.den);
    return part1 + part2;
}

__global__ __launch_bounds__(256) void berhu_max_kernel(const float* __restrict__ pred, const float* __restrict__ target, int64_t n,
                                                        unsigned* __restrict__ pmax) {
    __shared__ unsigned shu[4];
    unsigned m = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const float t = target[e];
        if (t > 0.f) {
            const unsigned b = __float_as_uint(fabsf(t - pred[e]));
            m = b > m ? b : m;
        }
    }
    m = block_max_u(m, shu);
    if (threadIdx.x == 0) pmax[blockIdx.x] = m;
}

// ---------------------------------------------------------------- the masked-sum pass and its final pass
// Evaluation metrics (evaluation/metrics.py:34-58), ten sums: count, sum d^2, sum |d|, sum |log10 o - log10 t|, sum |d|/t, #(r<1.25),
// #(r<1.25^2), #(r<1.25^3), sum (1/o-1/t)^2, sum |1/o-1/t|   over pixels with t > 0, d = o - t, r = max(o/t, t/o)
// the ten fp32 terms of one valid pixel: metric_terms (metric_terms.h)
enum : int { LOSS_NONE = 0, LOSS_L1, LOSS_L2, LOSS_BERHU };
// MaskedL1Loss: |t-p|; MaskedMSELoss (criteria_new.py:31-41): (t-p)^2; MaskedBerHuLoss: berhu_term
template <int LOSS>
__device__ __forceinline__ float loss_term(float diff, const BerhuConsts& k) {
    if constexpr (LOSS == LOSS_BERHU) return berhu_term(fabsf(diff), k);
    else if constexpr (LOSS == LOSS_L2) return diff * diff;
    else return fabsf(diff);
}
// ONE pass over the valid pixels (t > 0) of hw elements of (pred, target) for every loss and for the metrics that ride along with it,
// called by every thread of a block; a thread takes the elements e0, e0 + stride, ... (the kernel's grid-stride walk).  dst[(LOSS ? 2 : 0) + (MET ? 10 : 0)], this block's
// sums: the sum of the loss terms, the count, then the ten metric sums.  A column depends neither on LOSS nor on MET: the grid
// (red_grid(hw)), the per-thread element order and block_sum_d are the same in every form, so metrics riding along cannot move a
// bit of a loss, and a frame of hw elements is reduced exactly as a tensor of hw elements is.
template <int LOSS, bool MET>
__device__ __forceinline__ void masked_sums(const float* __restrict__ pred, const float* __restrict__ target, int64_t hw,
                                            int64_t e0, int64_t stride, const BerhuConsts& k, double* __restrict__ dst, double* sh) {
    constexpr int NL = LOSS != LOSS_NONE ? 2 : 0;
    double s = 0.0, c = 0.0;
    double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t e = e0; e < hw; e += stride) {
        const float t = target[e];
        if (t > 0.f) {
            const float o = pred[e];
            if constexpr (LOSS != LOSS_NONE) {
                s += (double)loss_term<LOSS>(t - o, k);
                c += 1.0;
            }
            if constexpr (MET) metric_terms(o, t, acc);
        }
    }
    if constexpr (LOSS != LOSS_NONE) {
        s = block_sum_d(s, sh);
        c = block_sum_d(c, sh);
        if (threadIdx.x == 0) {
            dst[0] = s;
            dst[1] = c;
        }
    }
    if constexpr (MET) {
        for (int i = 0; i < 10; ++i) {
            const double v = block_sum_d(acc[i], sh);
            if (threadIdx.x == 0) dst[NL + i] = v;
        }
    }
}
// The pass of every whole-tensor sums entry point: part[block][(LOSS ? 2 : 0) + (MET ? 10 : 0)].
// LOSS_BERHU: every block first reduces the maxima of berhu_max_kernel (one per block of this grid) and forms the three constants itself.
template <int LOSS, bool MET>
__global__ __launch_bounds__(256) void masked_pass_kernel(const float* __restrict__ pred, const float* __restrict__ target, int64_t n,
                                                          double thresh, const unsigned* __restrict__ pmax, double* __restrict__ part) {
    __shared__ double sh[4];
    BerhuConsts k = {};
    if constexpr (LOSS == LOSS_BERHU) {
        __shared__ unsigned shu[4];
        k = berhu_consts(thresh * (double)__uint_as_float(blocks_max_u(pmax, gridDim.x, shu)));
    }
    masked_sums<LOSS, MET>(pred, target, n, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, k, part + (size_t)blockIdx.x * ((LOSS != LOSS_NONE ? 2 : 0) + (MET ? 10 : 0)), sh);
}
// The blocks' partials added column by column, by every thread of one block of `threads` threads: part[nblocks][NA + NB], the first NA
// columns to out_a[NA], the others to out_b[NB]
template <int NA, int NB>
__device__ __forceinline__ void column_sums(const double* __restrict__ part, int nblocks, int threads, double* __restrict__ out_a,
                                            double* __restrict__ out_b, double* sh) {
    constexpr int stride = NA + NB;
    for (int k = 0; k < stride; ++k) {
        double s = 0.0;
        for (int i = threadIdx.x; i < nblocks; i += threads) s += part[(size_t)i * stride + k];
        s = block_sum_d(s, sh);
        if (threadIdx.x == 0) {
            if (k < NA) out_a[k] = s;
            else out_b[k - NA] = s;
        }
    }
}
// The final pass of every whole-tensor sums entry point (one workgroup).  pmax (BerHu): then out_a[NA] = delta, out_a[NA + 1] = the maximum.
template <int NA, int NB>
__global__ __launch_bounds__(256) void final_sums_kernel(const double* __restrict__ part, const unsigned* __restrict__ pmax, int nblocks,
                                                         double thresh, double* __restrict__ out_a, double* __restrict__ out_b) {
    __shared__ double sh[4];
    column_sums<NA, NB>(part, nblocks, blockDim.x, out_a, out_b, sh);
    if (pmax) {                                                                // (grid-uniform)
        __shared__ unsigned shu[4];
        const double m = (double)__uint_as_float(blocks_max_u(pmax, nblocks, shu));
        if (threadIdx.x == 0) {
            out_a[NA] = thresh * m;
            out_a[NA + 1] = m;
        }
    }
}
// per-frame metric sums: grid (blocks per frame, frames), part[frame][block][10], then one workgroup per frame.  Kernels of their own
// over masked_sums and column_sums: launched through the whole-tensor kernels' wider argument lists, rd_depth_metrics_frames measured
// 0.4 us slower than with these.
__global__ __launch_bounds__(256) void metrics_frames_partial_kernel(const float* __restrict__ out, const float* __restrict__ target,
                                                                     int64_t hw, double* __restrict__ part) {
    __shared__ double sh[4];
    masked_sums<LOSS_NONE, true>(out + (size_t)blockIdx.y * hw, target + (size_t)blockIdx.y * hw, hw,
                                 (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, BerhuConsts{},
                                 part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 10, sh);
}
__global__ __launch_bounds__(256) void metrics_frames_final_kernel(const double* __restrict__ part, int nb, double* __restrict__ sums) {
    __shared__ double sh[4];
    column_sums<0, 10>(part + (size_t)blockIdx.x * nb * 10, nb, blockDim.x, nullptr, sums + (size_t)blockIdx.x * 10, sh);
}

// autograd of the reference's expression in its own fp32 steps: g = coef / count reaches diff through part1 (where in1) and through
// part2 as (g / den) * (2 diff) (where in2); |.|' is 0 at t == p
__global__ __launch_bounds__(256) void berhu_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, int64_t n,
                                                        const double* __restrict__ sums, const float* __restrict__ coef,
                                                        float* __restrict__ dpred, int accumulate) {
#pragma clang fp contract(off)
    const float k = (float)((double)coef[0] / sums[1]);
    const BerhuConsts c = berhu_consts(sums[2]);
    const float kd = __fdiv_rn(k, c.den);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const float t = target[e];
        float g = 0.f;
        if (t > 0.f) {
            const float d = t - pred[e];
            const float diff = fabsf(d);
            bool in1, in2;
            berhu_branches(diff, c, in1, in2);
            float a = in1 ? k : 0.f;
            if (in2) a = a + kd * (2.f * diff);
            g = d > 0.f ? -a : (d < 0.f ? a : 0.f);
        }
        dpred[e] = accumulate ? dpred[e] + g : g;
    }
}

// ---------------------------------------------------------------- device-resident AverageMeter (evaluation/metrics.py:179-216)
// The ten metrics of one row of sums: meter_metric (metric_terms.h).
// One workgroup, no atomics: thread (g, j) owns word j of meter g -- j = 0 the count, 1..10 the weighted metric sums, 11 the number of
// updates -- and walks the rows in order; the first ten threads also keep the latest row's metrics.
__global__ __launch_bounds__(256) void meter_update_kernel(const double* __restrict__ sums, int rows, const double* __restrict__ weights,
                                                           const int32_t* __restrict__ groups, int n_groups, double* __restrict__ meter,
                                                           double* __restrict__ last) {
    for (int i = threadIdx.x; i < n_groups * 12; i += blockDim.x) {
        const int g = i / 12, j = i - g * 12;
        double v = meter[i];
        for (int r = 0; r < rows; ++r) {
            const int32_t mask = groups ? groups[r] : 1;
            if (!((mask >> g) & 1)) continue;
            const double w = weights ? weights[r] : 1.0;
            if (j == 0) v += w;
            else if (j == 11) v += 1.0;
            else v += w * meter_metric(sums + (size_t)r * 10, j - 1);
        }
        meter[i] = v;
    }
    if (threadIdx.x < 10) last[threadIdx.x] = meter_metric(sums + (size_t)(rows - 1) * 10, threadIdx.x);
}

// ---------------------------------------------------------------- smoothness
// pass 1: per-sample sum of pred -> part[n][block]
__global__ __launch_bounds__(256) void smooth_sum_kernel(const float* __restrict__ pred, int64_t hw, double* __restrict__ part) {
    __shared__ double sh[4];
    const int n = blockIdx.y;
    const float* p = pred + (size_t)n * hw;
    double s = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < hw; e += (int64_t)gridDim.x * blockDim.x) s += (double)p[e];
    s = block_sum_d(s, sh);
    if (threadIdx.x == 0) part[(size_t)n * gridDim.x + blockIdx.x] = s;
}
// scal[n] = mean + 1e-7 (as the reference computes it in fp32: mean(2).mean(3) then + 1e-7)
__global__ __launch_bounds__(256) void smooth_mean_kernel(const double* __restrict__ part, int nb, int64_t hw, float* __restrict__ sden) {
    __shared__ double sh[4];
    const int n = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) s += part[(size_t)n * nb + i];
    s = block_sum_d(s, sh);
    if (threadIdx.x == 0) sden[n] = (float)(s / (double)hw) + 1e-7f;
}

__device__ __forceinline__ float edge_w(const float* __restrict__ img, int C, int64_t hw, int64_t a, int64_t b) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += fabsf(img[c * hw + a] - img[c * hw + b]);
    return expf(-s / (float)C);
}
__device__ __forceinline__ float sgn(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }
// Normalised depth of one pixel, rounded ONCE.  Left to itself the compiler contracts the product into the subtraction that follows:
// fma(-p1, inv, d0) subtracts an unrounded product from a rounded one, so two EQUAL neighbours differed by d0's rounding error and a
// tie -- every flat region of a prediction -- got a sign (+-w/count in the gradient) where the reference's |.|' is 0.  The empty asm
// makes the rounded product a value of its own (HIP's __fmul_rn is a plain multiplication and contracts like one).
__device__ __forceinline__ float norm_depth(float p, float inv) {
    float r = p * inv;
    asm volatile("" : "+v"(r));
    return r;
}

// pass 2: q[n,y,x] = dL/d(dhat) ; partial sums (loss_x, loss_y, sum q*pred) per block
__global__ __launch_bounds__(256) void smooth_main_kernel(const float* __restrict__ pred, const float* __restrict__ image, int N,
                                                          int C, int H, int W, const float* __restrict__ sden,
                                                          float* __restrict__ q, double* __restrict__ part) {
    __shared__ double sh[4];
    const int n = blockIdx.y;
    const int64_t hw = (int64_t)H * W;
    const float* p = pred + (size_t)n * hw;
    const float* img = image + (size_t)n * C * hw;
    const float inv = 1.f / sden[n];
    const float inx = 1.f / ((float)N * H * (W - 1)), iny = 1.f / ((float)N * (H - 1) * W);
    double lx = 0.0, ly = 0.0, tq = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < hw; e += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)((unsigned)e / (unsigned)W), x = (int)((unsigned)e - (unsigned)y * (unsigned)W);   // (one image: e < 2^31, checked by the host)
        const float d = norm_depth(p[e], inv);
        float qq = 0.f;
        if (x + 1 < W) {
            const float w = edge_w(img, C, hw, e, e + 1);
            const float diff = d - norm_depth(p[e + 1], inv);
            lx += (double)(fabsf(diff) * w);
            qq += w * sgn(diff) * inx;
        }
        if (x > 0) {
            const float w = edge_w(img, C, hw, e - 1, e);
            qq -= w * sgn(norm_depth(p[e - 1], inv) - d) * inx;
        }
        if (y + 1 < H) {
            const float w = edge_w(img, C, hw, e, e + W);
            const float diff = d - norm_depth(p[e + W], inv);
            ly += (double)(fabsf(diff) * w);
            qq += w * sgn(diff) * iny;
        }
        if (y > 0) {
            const float w = edge_w(img, C, hw, e - W, e);
            qq -= w * sgn(norm_depth(p[e - W], inv) - d) * iny;
        }
        q[(size_t)n * hw + e] = qq;
        tq += (double)qq * (double)p[e];
    }
    lx = block_sum_d(lx, sh);
    ly = block_sum_d(ly, sh);
    tq = block_sum_d(tq, sh);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)n * gridDim.x + blockIdx.x) * 3;
        o[0] = lx; o[1] = ly; o[2] = tq;
    }
}
// out[0] = loss ; tsum[n] = sum_k q_k p_k
__global__ __launch_bounds__(256) void smooth_final_kernel(const double* __restrict__ part, int N, int nb, int H, int W,
                                                           double* __restrict__ out, double* __restrict__ tsum) {
    __shared__ double sh[4];
    double LX = 0.0, LY = 0.0;
    for (int n = 0; n < N; ++n) {
        double lx = 0.0, ly = 0.0, t = 0.0;
        for (int i = threadIdx.x; i < nb; i += blockDim.x) {
            const double* o = part + ((size_t)n * nb + i) * 3;
            lx += o[0]; ly += o[1]; t += o[2];
        }
        lx = block_sum_d(lx, sh);
        ly = block_sum_d(ly, sh);
        t = block_sum_d(t, sh);
        LX += lx; LY += ly;
        if (threadIdx.x == 0) tsum[n] = t;
    }
    if (threadIdx.x == 0) out[0] = LX / ((double)N * H * (W - 1)) + LY / ((double)N * (H - 1) * W);
}
// dpred = coef * (q / s - T / (HW s^2))
__global__ __launch_bounds__(256) void smooth_bwd_kernel(const float* __restrict__ q, const float* __restrict__ sden,
                                                         const double* __restrict__ tsum, int64_t hw, const float* __restrict__ coef,
                                                         float* __restrict__ dpred, int accumulate) {
    const int n = blockIdx.y;
    const float k = coef[0];
    const float s = sden[n];
    const float a = k / s, b = (float)((double)k * tsum[n] / ((double)hw * (double)s * (double)s));
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < hw; e += (int64_t)gridDim.x * blockDim.x) {
        const size_t i = (size_t)n * hw + e;
        const float g = a * q[i] - b;
        dpred[i] = accumulate ? dpred[i] + g : g;
    }
}

// ---------------------------------------------------------------- filter layer / totals / optimizer
__global__ __launch_bounds__(256) void radar_filter_kernel(const float* __restrict__ x, int Ctot, int c, int64_t hw, int N,
                                                           const float* __restrict__ dense, float* __restrict__ kept,
                                                           float* __restrict__ mask, float log_ratio, float log_alpha) {
    const int64_t total = (int64_t)N * hw;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = e / hw, r = e - n * hw;
        const float sp = x[((size_t)n * Ctot + c) * hw + r];
        const float de = dense[e];
        const float thr = expf(((de * log_ratio) / 100.0f) + log_alpha);
        const float m = fabsf(de - sp) <= thr ? 1.f : 0.f;
        kept[e] = sp * m;
        mask[e] = m;
    }
}

__global__ void uncertainty_total_kernel(const double* s1, const double* s2, const double* sm, const float* w1, const float* w2,
                                         float w_smooth, float* loss4, float* coefs3, float* dw1, float* dw2) {
    const double d1 = s1[0] / s1[1], d2 = s2[0] / s2[1], s = sm[0];
    const double e1 = exp(-(double)w1[0]), e2 = exp(-(double)w2[0]);
    const double st1 = d1 + (double)w_smooth * s;
    loss4[0] = (float)d1; loss4[1] = (float)d2; loss4[2] = (float)s;
    loss4[3] = (float)(e1 * st1 + e2 * d2 + (double)w1[0] + (double)w2[0]);
    coefs3[0] = (float)e1; coefs3[1] = (float)(w_smooth * e1); coefs3[2] = (float)e2;
    dw1[0] = (float)(1.0 - e1 * st1);
    dw2[0] = (float)(1.0 - e2 * d2);
}
__global__ void l1_total_kernel(const double* sums, float* loss, float* coef) {
    loss[0] = (float)(sums[0] / sums[1]);
    coef[0] = 1.f;
}

// ---------------------------------------------------------------- optimizer: sum of squares of the gradient, SGD
// (the clip that joins the two: clip_prologue, step_tail.h)
__device__ __forceinline__ double sumsq4(double a, const float4 v) {
    a = fma((double)v.x, (double)v.x, a);
    a = fma((double)v.y, (double)v.y, a);
    a = fma((double)v.z, (double)v.z, a);
    return fma((double)v.w, (double)v.w, a);
}
// The square of an fp32 value is exact in float64 (48 significant bits, at most 2^256), and 1.5e7 of them -- 2^31 of them -- cannot
// overflow it: the sum is finite exactly when every element is finite.  The skip decision of clip_prologue rests on that.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n4, int64_t n, double* __restrict__ part) {
    __shared__ double sh[4];
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double a = 0.0;
    for (; e + 3 * stride < n4; e += 4 * stride) {          // four 16-byte loads in flight per lane; added in the order of the plain loop
        const float4 v0 = g4[e], v1 = g4[e + stride], v2 = g4[e + 2 * stride], v3 = g4[e + 3 * stride];
        a = sumsq4(sumsq4(sumsq4(sumsq4(a, v0), v1), v2), v3);
    }
    for (; e < n4; e += stride) a = sumsq4(a, g4[e]);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const float x = g[(n4 << 2) + threadIdx.x];
        a = fma((double)x, (double)x, a);
    }
    a = block_total_d(a, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

__device__ __forceinline__ float fma_s(float a, float x, float y) { return fmaf(a, x, y); }
__device__ __forceinline__ float4 fma_s(float a, const float4 x, const float4 y) {
    return make_float4(fmaf(a, x.x, y.x), fmaf(a, x.y, y.y), fmaf(a, x.z, y.z), fmaf(a, x.w, y.w));
}
// torch.optim.SGD with momentum and weight decay (main.py:285-290,445) on one 16-byte word (V = float4) or one tail element (V = float):
// d = wd p + s g; b = d on the first step (no momentum buffer yet: buf is not read), momentum b + d after it; p -= lr b.  ONE
// definition for the loop and the tail of both SGD kernels, so that a coefficient of 1.0f (s = gscale) gives the unclipped
// step's bits.
template <class V>
__device__ __forceinline__ void sgd_update(V* __restrict__ p, const V* __restrict__ g, V* __restrict__ buf, float lr, float momentum,
                                           float wd, float s, bool first) {
    V pv = *p;
    V b = fma_s(wd, pv, s * *g);
    if (!first) b = fma_s(momentum, *buf, b);
    *buf = b;
    pv -= lr * b;
    *p = pv;
}
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                  int64_t n4, int64_t n, float lr, float momentum, float wd, float gscale, int first) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x)
        sgd_update(reinterpret_cast<float4*>(p) + e, reinterpret_cast<const float4*>(g) + e, reinterpret_cast<float4*>(buf) + e, lr, momentum,
                   wd, gscale, first);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t e = (n4 << 2) + threadIdx.x;
        sgd_update(p + e, g + e, buf + e, lr, momentum, wd, gscale, first);
    }
}
// sgd_kernel's walk over sgd_update (a momentum buffer always exists: first = 0) with gscale * coef in place of gscale.  Every block
// forms S, the norm and the coefficient from the partials (clip_prologue).  A kernel of its own: as one template with sgd_kernel both
// entry points measured 0.2 us slower than the parent's kernels.  Each kernel reads blockDim.x / gridDim.x itself (read in an inlined
// device function they compile through the non-uniform-workgroup path), so the walk is written in both.
__global__ __launch_bounds__(256) void sgd_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                       int64_t n4, int64_t n, float lr, float momentum, float wd, float gscale,
                                                       double max_norm, int skip_nonfinite, const double* __restrict__ part, int n_part,
                                                       double* __restrict__ stats) {
    __shared__ double sh[4];
    const ClipDecision c = clip_prologue(gscale, ClipArgs{max_norm, skip_nonfinite, part, n_part, stats}, sh);
    if (c.skip) return;                                                        // (block-uniform) before anything of p or buf is touched
    const float s = gscale * c.coef;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x)
        sgd_update(reinterpret_cast<float4*>(p) + e, reinterpret_cast<const float4*>(g) + e, reinterpret_cast<float4*>(buf) + e, lr, momentum,
                   wd, s, false);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t e = (n4 << 2) + threadIdx.x;
        sgd_update(p + e, g + e, buf + e, lr, momentum, wd, s, false);
    }
}

constexpr int SM_BLOCKS = 256;  // blocks per sample in the smoothness passes (64 left the b = 8 passes of config 4 at two blocks per CU: smooth_main 157 us)

}  // namespace rd
using namespace rd;

extern "C" int rd_loss_tiles(int64_t n) { return red_grid(n); }

// The launches of every whole-tensor sums entry point (the argument checks are the entry point's own): berhu_max_kernel for LOSS_BERHU,
// the masked pass, the final pass.  ws: doubles part[tiles][2 (a loss) + 10 (MET)], tiles = rd_loss_tiles(n); LOSS_BERHU: unsigned
// pmax[tiles] at part + 12 * tiles, with and without metrics.  sums[2] (BerHu: [4]) and msums[10]; a form without a loss or without
// metrics does not touch its pointer.
template <int LOSS, bool MET>
static int launch_sums(const float* pred, const float* target, int64_t n, double thresh, float* ws, double* sums, double* msums,
                       void* stream) {
    const auto launched = [](const char* kernel) {                             // a launch failure names the instantiation
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            set_error("%s<%s, %s>: %s", kernel, LOSS == LOSS_NONE ? "none" : LOSS == LOSS_L1 ? "L1" : LOSS == LOSS_L2 ? "L2" : "BerHu",
                      MET ? "metrics" : "no metrics", hipGetErrorString(e));
        return e == hipSuccess;
    };
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int g = red_grid(n);
    constexpr int NL = LOSS != LOSS_NONE ? 2 : 0;
    double* part = reinterpret_cast<double*>(ws);
    unsigned* pmax = nullptr;
    if constexpr (LOSS == LOSS_BERHU) {
        pmax = reinterpret_cast<unsigned*>(part + (size_t)12 * g);
        hipLaunchKernelGGL(berhu_max_kernel, dim3(g), dim3(256), 0, s, pred, target, n, pmax);
        RD_CHECK_LAUNCH("berhu_max_kernel");
    }
    hipLaunchKernelGGL((masked_pass_kernel<LOSS, MET>), dim3(g), dim3(256), 0, s, pred, target, n, thresh, pmax, part);
    if (!launched("masked_pass_kernel")) return RD_ELAUNCH;
    hipLaunchKernelGGL((final_sums_kernel<NL, MET ? 10 : 0>), dim3(1), dim3(256), 0, s, part, pmax, g, thresh, sums, msums);
    if (!launched("final_sums_kernel")) return RD_ELAUNCH;
    return RD_OK;
}

// sums[0] = sum |t-p| over t>0, sums[1] = count.  ws: 2*rd_loss_tiles(n) doubles (pass as float* with 4*tiles floats, 8-byte aligned)
extern "C" int rd_masked_l1_sums(const float* pred, const float* target, int64_t n, float* ws, double* sums, void* stream) {
    RD_CHECK_ARG(pred && target && ws && sums && n > 0 && ((uintptr_t)ws & 7) == 0, "masked_l1_sums: bad arguments");
    return launch_sums<LOSS_L1, false>(pred, target, n, 0.0, ws, sums, nullptr, stream);
}
// MaskedMSELoss (criteria_new.py:31-41): sums[0] = sum (t-p)^2 over t>0, sums[1] = count
extern "C" int rd_masked_l2_sums(const float* pred, const float* target, int64_t n, float* ws, double* sums, void* stream) {
    RD_CHECK_ARG(pred && target && ws && sums && n > 0 && ((uintptr_t)ws & 7) == 0, "masked_l2_sums: bad arguments");
    return launch_sums<LOSS_L2, false>(pred, target, n, 0.0, ws, sums, nullptr, stream);
}

// sums[10] as listed above; ws: 10*rd_loss_tiles(n) doubles
extern "C" int rd_depth_metrics(const float* output, const float* target, int64_t n, float* ws, double* sums, void* stream) {
    RD_CHECK_ARG(output && target && ws && sums && n > 0 && ((uintptr_t)ws & 7) == 0, "depth_metrics: bad arguments");
    return launch_sums<LOSS_NONE, true>(output, target, n, 0.0, ws, nullptr, sums, stream);
}

// Loss sums and metric sums in one pass over pred / target: sums[2] exactly as rd_masked_l1_sums / rd_masked_l2_sums write them,
// msums[10] as rd_depth_metrics lists them.  ws: 12*rd_loss_tiles(n) doubles
extern "C" int rd_masked_l1_sums_metrics(const float* pred, const float* target, int64_t n, float* ws, double* sums, double* msums,
                                         void* stream) {
    RD_CHECK_ARG(pred && target && ws && sums && msums && n > 0 && ((uintptr_t)ws & 7) == 0, "masked_l1_sums_metrics: bad arguments");
    return launch_sums<LOSS_L1, true>(pred, target, n, 0.0, ws, sums, msums, stream);
}
extern "C" int rd_masked_l2_sums_metrics(const float* pred, const float* target, int64_t n, float* ws, double* sums, double* msums,
                                         void* stream) {
    RD_CHECK_ARG(pred && target && ws && sums && msums && n > 0 && ((uintptr_t)ws & 7) == 0, "masked_l2_sums_metrics: bad arguments");
    return launch_sums<LOSS_L2, true>(pred, target, n, 0.0, ws, sums, msums, stream);
}

// sums[frames][10]: the ten sums of rd_depth_metrics for every frame of a [frames,1,H,W] pair (hw = H*W); a frame without a valid
// pixel gets a row of zeros.  ws: rd_depth_metrics_frames_workspace_floats(frames, hw) floats, 8-byte aligned
extern "C" int64_t rd_depth_metrics_frames_workspace_floats(int32_t frames, int64_t hw) {
    if (frames <= 0 || hw <= 0) return 0;
    return 2 * (int64_t)frames * red_grid(hw) * 10;
}
extern "C" int rd_depth_metrics_frames(const float* output, const float* target, int32_t frames, int64_t hw, float* ws, double* sums,
                                       void* stream) {
    RD_CHECK_ARG(output && target && ws && sums && frames > 0 && hw > 0 && ((uintptr_t)ws & 7) == 0, "depth_metrics_frames: bad arguments");
    RD_CHECK_ARG(frames <= 65535, "depth_metrics_frames: at most 65535 frames per call, got %d", frames);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int g = red_grid(hw);
    double* part = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(metrics_frames_partial_kernel, dim3(g, frames), dim3(256), 0, s, output, target, hw, part);
    RD_CHECK_LAUNCH("metrics_frames_partial_kernel");
    hipLaunchKernelGGL(metrics_frames_final_kernel, dim3(frames), dim3(256), 0, s, part, g, sums);
    RD_CHECK_LAUNCH("metrics_frames_final_kernel");
    return RD_OK;
}

// Result + AverageMeter.update on the device: each of `rows` rows of ten sums becomes the ten metrics (fp64) and is added, weighted
// by weights[row] (nullptr: 1), into every meter g < n_groups whose bit is set in groups[row] (nullptr: bit 0).
// meter[n_groups][12] = count, ten weighted sums in Result.update's order, number of updates; last[10] = the latest row's metrics.
extern "C" int rd_meter_update(const double* sums, int32_t rows, const double* weights, const int32_t* groups, int32_t n_groups,
                               double* meter, double* last, void* stream) {
    RD_CHECK_ARG(sums && meter && last && rows > 0, "meter_update: bad arguments");
    RD_CHECK_ARG(n_groups >= 1 && n_groups <= 31, "meter_update: n_groups must be 1..31 (one bit of an int32 mask each), got %d", n_groups);
    hipLaunchKernelGGL(meter_update_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), sums, rows, weights, groups,
                       n_groups, meter, last);
    RD_CHECK_LAUNCH("meter_update_kernel");
    return RD_OK;
}

extern "C" int rd_masked_l1_bwd(const float* pred, const float* target, int64_t n, const double* sums, const float* coef,
                                float* dpred, int32_t accumulate, void* stream) {
    RD_CHECK_ARG(pred && target && sums && coef && dpred && n > 0, "masked_l1_bwd: bad arguments");
    hipLaunchKernelGGL(l1_bwd_kernel<false>, dim3(ew_grid2(n)), dim3(256), 0, static_cast<hipStream_t>(stream), pred, target, n, sums, coef,
                       dpred, accumulate);
    RD_CHECK_LAUNCH("l1_bwd_kernel");
    return RD_OK;
}
// dpred = coef * 2 (pred - target) / count on valid pixels, 0 elsewhere
extern "C" int rd_masked_l2_bwd(const float* pred, const float* target, int64_t n, const double* sums, const float* coef,
                                float* dpred, int32_t accumulate, void* stream) {
    RD_CHECK_ARG(pred && target && sums && coef && dpred && n > 0, "masked_l2_bwd: bad arguments");
    hipLaunchKernelGGL(l1_bwd_kernel<true>, dim3(ew_grid2(n)), dim3(256), 0, static_cast<hipStream_t>(stream), pred, target, n, sums, coef,
                       dpred, accumulate);
    RD_CHECK_LAUNCH("l2_bwd_kernel");
    return RD_OK;
}

// MaskedBerHuLoss.  workspace layout: doubles part[tiles][12] (the plain call uses [tiles][2] of it) | unsigned pmax[tiles] (padded to even)
extern "C" int64_t rd_berhu_workspace_floats(int64_t n) {
    if (n < 1) return RD_EBERHU_RANGE;
    const int64_t g = red_grid(n);
    return 2 * 12 * g + ((g + 1) & ~(int64_t)1);
}
template <bool MET>
static int berhu_sums(const char* what, const float* pred, const float* target, int64_t n, double thresh, float* ws, double* sums,
                      double* msums, void* stream) {
    RD_CHECK_CODE(pred && target && ws && sums && (msums || !MET), RD_EBERHU_NULL, "%s: null argument", what);
    RD_CHECK_CODE(n >= 1, RD_EBERHU_RANGE, "%s: n = %lld, at least one element is needed", what, (long long)n);
    RD_CHECK_CODE(std::isfinite(thresh) && thresh > 0.0, RD_EBERHU_THRESH, "%s: thresh = %g has to be finite and positive", what, thresh);
    RD_CHECK_CODE((((uintptr_t)ws | (uintptr_t)sums | (uintptr_t)msums) & 7) == 0, RD_EBERHU_ALIGN,
                  "%s: the workspace and the sums have to be 8-byte aligned", what);
    return launch_sums<LOSS_BERHU, MET>(pred, target, n, thresh, ws, sums, msums, stream);
}
extern "C" int rd_masked_berhu_sums(const float* pred, const float* target, int64_t n, double thresh, float* ws, double* sums, void* stream) {
    return berhu_sums<false>("masked_berhu_sums", pred, target, n, thresh, ws, sums, nullptr, stream);
}
extern "C" int rd_masked_berhu_sums_metrics(const float* pred, const float* target, int64_t n, double thresh, float* ws, double* sums,
                                            double* msums, void* stream) {
    return berhu_sums<true>("masked_berhu_sums_metrics", pred, target, n, thresh, ws, sums, msums, stream);
}
extern "C" int rd_masked_berhu_bwd(const float* pred, const float* target, int64_t n, const double* sums, const float* coef, float* dpred,
                                   int32_t accumulate, void* stream) {
    RD_CHECK_CODE(pred && target && sums && coef && dpred, RD_EBERHU_NULL, "masked_berhu_bwd: null argument");
    RD_CHECK_CODE(n >= 1, RD_EBERHU_RANGE, "masked_berhu_bwd: n = %lld, at least one element is needed", (long long)n);
    RD_CHECK_CODE(((uintptr_t)sums & 7) == 0, RD_EBERHU_ALIGN, "masked_berhu_bwd: the sums have to be 8-byte aligned");
    hipLaunchKernelGGL(berhu_bwd_kernel, dim3(ew_grid2(n)), dim3(256), 0, static_cast<hipStream_t>(stream), pred, target, n, sums, coef,
                       dpred, accumulate);
    RD_CHECK_LAUNCH("berhu_bwd_kernel");
    return RD_OK;
}

// workspace layout (floats): q[N*H*W] | sden[N] (padded to even) | doubles: tsum[N], part[N*SM_BLOCKS*3]
extern "C" int64_t rd_smooth_workspace_floats(int32_t N, int32_t H, int32_t W) {
    const int64_t nhw = (int64_t)N * H * W;
    return ((nhw + 1) & ~(int64_t)1) + ((N + 1) & ~1) + 2 * ((int64_t)N + (int64_t)N * SM_BLOCKS * 3);
}

static void smooth_carve(float* ws, int N, int H, int W, float*& q, float*& sden, double*& tsum, double*& part) {
    const int64_t nhw = (int64_t)N * H * W;
    q = ws;
    sden = ws + ((nhw + 1) & ~(int64_t)1);
    tsum = reinterpret_cast<double*>(sden + ((N + 1) & ~1));
    part = tsum + N;
}

extern "C" int rd_smooth_fwd(const float* pred, const float* image, int32_t N, int32_t C, int32_t H, int32_t W, float* ws,
                             double* out, void* stream) {
    RD_CHECK_ARG(pred && image && ws && out && N > 0 && C > 0 && H > 1 && W > 1 && ((uintptr_t)ws & 7) == 0, "smooth_fwd: bad arguments");
    RD_CHECK_ARG((int64_t)H * W < (1ll << 31), "smooth_fwd: one image must have fewer than 2^31 pixels");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *q, *sden;
    double *tsum, *part;
    smooth_carve(ws, N, H, W, q, sden, tsum, part);
    const int64_t hw = (int64_t)H * W;
    hipLaunchKernelGGL(smooth_sum_kernel, dim3(SM_BLOCKS, N), dim3(256), 0, s, pred, hw, part);
    RD_CHECK_LAUNCH("smooth_sum_kernel");
    hipLaunchKernelGGL(smooth_mean_kernel, dim3(N), dim3(256), 0, s, part, SM_BLOCKS, hw, sden);
    RD_CHECK_LAUNCH("smooth_mean_kernel");
    hipLaunchKernelGGL(smooth_main_kernel, dim3(SM_BLOCKS, N), dim3(256), 0, s, pred, image, N, C, H, W, sden, q, part);
    RD_CHECK_LAUNCH("smooth_main_kernel");
    hipLaunchKernelGGL(smooth_final_kernel, dim3(1), dim3(256), 0, s, part, N, SM_BLOCKS, H, W, out, tsum);
    RD_CHECK_LAUNCH("smooth_final_kernel");
    return RD_OK;
}

extern "C" int rd_smooth_bwd(int32_t N, int32_t H, int32_t W, const float* ws, const float* coef, float* dpred, int32_t accumulate,
                             void* stream) {
    RD_CHECK_ARG(ws && coef && dpred && N > 0, "smooth_bwd: bad arguments");
    float *q, *sden;
    double *tsum, *part;
    smooth_carve(const_cast<float*>(ws), N, H, W, q, sden, tsum, part);
    const int64_t hw = (int64_t)H * W;
    hipLaunchKernelGGL(smooth_bwd_kernel, dim3(SM_BLOCKS, N), dim3(256), 0, static_cast<hipStream_t>(stream), q, sden, tsum, hw,
                       coef, dpred, accumulate);
    RD_CHECK_LAUNCH("smooth_bwd_kernel");
    return RD_OK;
}

extern "C" int rd_radar_filter(const float* x, int32_t N, int32_t Ctot, int32_t c, int64_t hw, const float* dense, float* kept,
                               float* mask, void* stream) {
    RD_CHECK_ARG(x && dense && kept && mask && N > 0 && c >= 0 && c < Ctot && hw > 0, "radar_filter: bad arguments");
    // fp32 constants exactly as the reference's 0-dim tensors evaluate them: log(18/5), log(5)
    const float log_ratio = logf(18.0f / 5.0f), log_alpha = logf(5.0f);
    hipLaunchKernelGGL(radar_filter_kernel, dim3(ew_grid2((int64_t)N * hw)), dim3(256), 0, static_cast<hipStream_t>(stream), x, Ctot,
                       c, hw, N, dense, kept, mask, log_ratio, log_alpha);
    RD_CHECK_LAUNCH("radar_filter_kernel");
    return RD_OK;
}

extern "C" int rd_uncertainty_total(const double* sums1, const double* sums2, const double* smooth, const float* w1, const float* w2,
                                    float w_smooth, float* loss4, float* coefs3, float* dw1, float* dw2, void* stream) {
    RD_CHECK_ARG(sums1 && sums2 && smooth && w1 && w2 && loss4 && coefs3 && dw1 && dw2, "uncertainty_total: null argument");
    hipLaunchKernelGGL(uncertainty_total_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), sums1, sums2, smooth, w1, w2,
                       w_smooth, loss4, coefs3, dw1, dw2);
    RD_CHECK_LAUNCH("uncertainty_total_kernel");
    return RD_OK;
}

extern "C" int rd_l1_total(const double* sums, float* loss, float* coef, void* stream) {
    RD_CHECK_ARG(sums && loss && coef, "l1_total: null argument");
    hipLaunchKernelGGL(l1_total_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), sums, loss, coef);
    RD_CHECK_LAUNCH("l1_total_kernel");
    return RD_OK;
}

extern "C" int rd_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float wd, float grad_scale,
                           int32_t first_step, void* stream) {
    RD_CHECK_ARG(p && g && buf && n > 0 && ((uintptr_t)p & 15) == 0 && ((uintptr_t)g & 15) == 0 && ((uintptr_t)buf & 15) == 0,
                 "sgd_step: bad arguments (arenas must be 16-byte aligned)");
    hipLaunchKernelGGL(sgd_kernel, dim3(ew_grid2(n / 4 + 1)), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, buf, n / 4, n, lr,
                       momentum, wd, grad_scale, first_step);
    RD_CHECK_LAUNCH("sgd_kernel");
    return RD_OK;
}

// One double per block of grad_sumsq_kernel: a function of n alone (never of the CU count), so every device forms the same partials.
extern "C" int rd_grad_sumsq_partials(int64_t n) { return n > 0 ? red_grid(n) : 0; }

extern "C" int rd_grad_sumsq(const float* g, int64_t n, double* partials, void* stream) {
    RD_CHECK_ARG(g && partials && n > 0 && aligned16(g) && aligned16(partials),
                 "grad_sumsq: bad arguments (the arena and the partials must be 16-byte aligned)");
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(red_grid(n)), dim3(256), 0, static_cast<hipStream_t>(stream), g, n / 4, n, partials);
    RD_CHECK_LAUNCH("grad_sumsq_kernel");
    return RD_OK;
}

extern "C" int rd_sgd_step_clip(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float wd, float grad_scale,
                                double max_norm, int32_t skip_nonfinite, const double* partials, int32_t n_partials, double* stats,
                                void* stream) {
    RD_CHECK_ARG(p && g && buf && partials && stats && n > 0, "sgd_step_clip: null argument or n < 1");
    RD_CHECK_ARG(aligned16(p) && aligned16(g) && aligned16(buf) && aligned16(partials) && aligned16(stats),
                 "sgd_step_clip: the arenas, the partials and the stats must be 16-byte aligned");
    RD_CHECK_ARG(n_partials == red_grid(n), "sgd_step_clip: n_partials = %d, rd_grad_sumsq_partials(%lld) = %d", n_partials, (long long)n,
                 red_grid(n));
    hipLaunchKernelGGL(sgd_clip_kernel, dim3(ew_grid2(n / 4 + 1)), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, buf, n / 4, n, lr,
                       momentum, wd, grad_scale, max_norm, skip_nonfinite, partials, n_partials, stats);
    RD_CHECK_LAUNCH("sgd_clip_kernel");
    return RD_OK;
}
