// torch.optim.Adam / AdamW (single-tensor form, amsgrad and maximize off) over the flat arenas, with the optimizer state on the device.
//
// The step count, the running powers of the betas and the hyper-parameters live in a block of RD_ADAM_BLOCK_WORDS float64 words
// (layout: include/radar_depth_hip.h).  The host only ever writes to the block; adam_prepare_kernel (one workgroup) advances it and leaves
// the scalars of the step, each rounded to fp32 once, for adam_step_kernel, which only reads it: no workgroup reads a word that
// another workgroup of the same launch writes.  The skip decision of a non-finite step is taken in the prepare launch, so a skipped
// step advances nothing -- not t, not the products, not one element of p, m, v.
//
// Every fp32 operation of the update is an operation of its own (no contraction anywhere in this file, no fmaf), the division and the
// square root are the correctly rounded ones: a numpy float32 restatement reproduces the launch bit for bit (tests/adam_ref.py).
#include "step_tail.h"

#pragma clang fp contract(off)

namespace rd {
namespace {

enum : int { W_LR = 0, W_BETA1, W_BETA2, W_EPS, W_WD, W_T, W_B1T, W_B2T, W_SKIP, W_S, W_WDF, W_DECAY, W_OMB1, W_BETA2F, W_OMB2, W_BC2S,
             W_EPSF, W_STEP };
static_assert(W_STEP < RD_ADAM_BLOCK_WORDS, "the state block holds every word");

// The norm, the coefficient and the skip decision as the clipped SGD kernel forms them (clip_prologue, n_part > 0), then the advance of
// the block.
__global__ __launch_bounds__(256) void adam_prepare_kernel(double* __restrict__ blk, float gscale, ClipArgs clip) {
    __shared__ double sh[4];
    ClipDecision d = {1.f, false};
    if (clip.n_part > 0) d = clip_prologue(gscale, clip, sh);                  // (uniform: every lane takes part in the sum)
    if (threadIdx.x != 0) return;
    blk[W_SKIP] = d.skip ? 1.0 : 0.0;
    if (d.skip) return;                                                         // t, the products and the step's scalars stay as they were
    const double lr = blk[W_LR], b1 = blk[W_BETA1], b2 = blk[W_BETA2], eps = blk[W_EPS], wd = blk[W_WD];
    const double t = blk[W_T] + 1.0, b1t = blk[W_B1T] * b1, b2t = blk[W_B2T] * b2;
    blk[W_T] = t;
    blk[W_B1T] = b1t;
    blk[W_B2T] = b2t;
    blk[W_S] = (double)(gscale * d.coef);                                      // one fp32 product, as in the clipped SGD kernel
    blk[W_WDF] = (double)(float)wd;
    blk[W_DECAY] = (double)(float)(1.0 - lr * wd);
    blk[W_OMB1] = (double)(float)(1.0 - b1);
    blk[W_BETA2F] = (double)(float)b2;
    blk[W_OMB2] = (double)(float)(1.0 - b2);
    blk[W_BC2S] = (double)(float)sqrt(1.0 - b2t);
    blk[W_EPSF] = (double)(float)eps;
    blk[W_STEP] = (double)(float)(lr / (1.0 - b1t));
}

struct AdamScalars {
    float s, wd, decay, omb1, beta2, omb2, bc2s, eps, step;
};

// hipcc's __fsqrt_rn is the 1-ulp hardware square root unless the whole translation unit is built with OCML_BASIC_ROUNDED_OPERATIONS;
// the plain operators are the IEEE round-to-nearest division and square root (the toolchain's default for fp32), which is what the
// restatement needs.
__device__ __forceinline__ float div_rn(float a, float b) { return a / b; }
__device__ __forceinline__ float sqrt_rn(float a) { return __builtin_sqrtf(a); }

// FORM 0: no weight decay; 1: coupled (Adam: g += wd p); 2: decoupled (AdamW: p *= 1 - lr wd)
template <int FORM>
__device__ __forceinline__ void adam_element(float& p, const float grad, float& m, float& v, const AdamScalars& k) {
    float g = k.s * grad;
    if (FORM == 1) g = g + k.wd * p;
    if (FORM == 2) p = p * k.decay;
    m = m + k.omb1 * (g - m);
    v = k.beta2 * v + (k.omb2 * g) * g;
    const float d = div_rn(sqrt_rn(v), k.bc2s) + k.eps;
    p = p - k.step * div_rn(m, d);
}

template <int FORM>
__device__ __forceinline__ void adam_stream(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                            int64_t n4, int64_t n, const AdamScalars& k) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        float4 pv = reinterpret_cast<float4*>(p)[e];
        const float4 gv = reinterpret_cast<const float4*>(g)[e];
        float4 mv = reinterpret_cast<float4*>(m)[e];
        float4 vv = reinterpret_cast<float4*>(v)[e];
        adam_element<FORM>(pv.x, gv.x, mv.x, vv.x, k);
        adam_element<FORM>(pv.y, gv.y, mv.y, vv.y, k);
        adam_element<FORM>(pv.z, gv.z, mv.z, vv.z, k);
        adam_element<FORM>(pv.w, gv.w, mv.w, vv.w, k);
        reinterpret_cast<float4*>(m)[e] = mv;
        reinterpret_cast<float4*>(v)[e] = vv;
        reinterpret_cast<float4*>(p)[e] = pv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t e = (n4 << 2) + threadIdx.x;
        float pe = p[e], me = m[e], ve = v[e];
        adam_element<FORM>(pe, g[e], me, ve, k);
        m[e] = me;
        v[e] = ve;
        p[e] = pe;
    }
}

__global__ __launch_bounds__(256) void adam_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, int64_t n4, int64_t n, int decoupled,
                                                        const double* __restrict__ blk) {
    if (blk[W_SKIP] != 0.0) return;                                            // (grid-uniform) before anything of p, m or v is touched
    // every word holds an fp32 value: the conversions are exact
    const AdamScalars k = {(float)blk[W_S],      (float)blk[W_WDF],  (float)blk[W_DECAY], (float)blk[W_OMB1], (float)blk[W_BETA2F],
                           (float)blk[W_OMB2],   (float)blk[W_BC2S], (float)blk[W_EPSF],  (float)blk[W_STEP]};
    if (k.wd == 0.f) adam_stream<0>(p, g, m, v, n4, n, k);                     // torch tests weight_decay != 0
    else if (!decoupled) adam_stream<1>(p, g, m, v, n4, n, k);
    else adam_stream<2>(p, g, m, v, n4, n, k);
}

}  // namespace
}  // namespace rd
using namespace rd;

extern "C" int rd_adam_prepare(double* block, int64_t n, float grad_scale, double max_norm, int32_t skip_nonfinite, const double* partials,
                               int32_t n_partials, double* stats, void* stream) {
    RD_CHECK_ARG(block && n > 0, "rd_adam_prepare: null state block or n < 1");
    RD_CHECK_ARG(aligned16(block) && aligned16(partials) && aligned16(stats), "rd_adam_prepare: the block, the partials and the stats must be 16-byte aligned");
    RD_CHECK_ARG((partials == nullptr) == (n_partials == 0) && (partials == nullptr || stats != nullptr),
                 "rd_adam_prepare: partials and stats come together with n_partials > 0, or not at all with n_partials = 0");
    RD_CHECK_ARG(n_partials == 0 || n_partials == rd_grad_sumsq_partials(n), "rd_adam_prepare: n_partials = %d, rd_grad_sumsq_partials(%lld) = %d",
                 n_partials, (long long)n, rd_grad_sumsq_partials(n));
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), block, grad_scale,
                       ClipArgs{max_norm, skip_nonfinite, partials, n_partials, stats});
    RD_CHECK_LAUNCH("adam_prepare_kernel");
    return RD_OK;
}

extern "C" int rd_adam_step(float* p, const float* g, float* m, float* v, int64_t n, int32_t mode, const double* block, void* stream) {
    RD_CHECK_ARG(p && g && m && v && block && n > 0, "rd_adam_step: null argument or n < 1");
    RD_CHECK_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(block),
                 "rd_adam_step: the arenas and the state block must be 16-byte aligned");
    RD_CHECK_ARG(mode == RD_ADAM || mode == RD_ADAMW, "rd_adam_step: mode %d is neither RD_ADAM (0) nor RD_ADAMW (1)", mode);
    hipLaunchKernelGGL(adam_step_kernel, dim3(ew_grid2(n / 4 + 1)), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, m, v, n / 4, n,
                       mode == RD_ADAMW ? 1 : 0, block);
    RD_CHECK_LAUNCH("adam_step_kernel");
    return RD_OK;
}
