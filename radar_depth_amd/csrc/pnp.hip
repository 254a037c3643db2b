// PnP-Depth refinement (Wang et al., "Plug-and-Play: Improve Depth Estimation via Sparse Data Propagation"): the two streaming
// kernels the eval-mode backward of the network's rear half needs beside the input-gradient convolutions.
//
//   rd_act_gate_t   out = dy where y > 0, 0 elsewhere: the ReLU of a folded conv + BatchNorm (+ residual), gated by the activation
//                   the eval forward keeps.  Channel slices of NHWC tensors (an UpProj module's halves), in place or out of place.
//   rd_pnp_update   z = z - alpha * sign(g), alpha read on the device.
//
// Both are HBM-bound (two reads and one write of 4 bytes per element, one compare): 16-byte accesses in the form of
// bn_act_kernel (norm_act.hip) where the channel count, the three channel strides and the base pointers allow, one element per
// thread otherwise (odd channel counts, slices at odd offsets: the kernel-level tests, no layer of the shipped networks).
#include "common.h"

namespace rd {

// dy and out are not __restrict__: out == dy is the in-place form
__global__ __launch_bounds__(256) void act_gate_kernel4(const float* dy, int lddy, const float* __restrict__ y, int ldy, float* out, int ldo,
                                                        int64_t M, int C) {
    const int Q = C >> 2;
    const int lq = quad_log2(Q);
    const int64_t total = M * Q;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        int64_t r;
        int c;
        split_quad(e, Q, lq, r, c);
        float4 g = ld4(dy + r * lddy + c);
        const float4 v = ld4(y + r * ldy + c);
        g.x = v.x > 0.f ? g.x : 0.f; g.y = v.y > 0.f ? g.y : 0.f; g.z = v.z > 0.f ? g.z : 0.f; g.w = v.w > 0.f ? g.w : 0.f;
        st4(out + r * ldo + c, g);
    }
}

__global__ __launch_bounds__(256) void act_gate_kernel1(const float* dy, int lddy, const float* __restrict__ y, int ldy, float* out, int ldo,
                                                        int64_t M, int C) {
    const int64_t total = M * C;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / C;
        const int c = (int)(e - r * C);
        out[r * ldo + c] = y[r * ldy + c] > 0.f ? dy[r * lddy + c] : 0.f;
    }
}

// torch.sign on the bits of g (no dependence on the kernel's denormal mode): +-0 -> 0, NaN -> NaN, everything else +-1.
// alpha * s is exact, so z - alpha * s is ONE fp32 rounding however the compiler contracts it.
__device__ __forceinline__ float pnp_step(float z, float g, float alpha) {
    const unsigned u = __float_as_uint(g), mag = u & 0x7fffffffu;
    const float s = mag == 0u ? 0.f : mag > 0x7f800000u ? g : (u >> 31) ? -1.f : 1.f;
    return z - alpha * s;
}

__global__ __launch_bounds__(256) void pnp_update_kernel4(float* __restrict__ z, int ldz, const float* __restrict__ g, int ldg, int64_t M, int C,
                                                          const float* __restrict__ alpha_dev) {
    const float alpha = alpha_dev[0];
    const int Q = C >> 2;
    const int lq = quad_log2(Q);
    const int64_t total = M * Q;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        int64_t r;
        int c;
        split_quad(e, Q, lq, r, c);
        float4 v = ld4(z + r * ldz + c);
        const float4 d = ld4(g + r * ldg + c);
        v.x = pnp_step(v.x, d.x, alpha); v.y = pnp_step(v.y, d.y, alpha); v.z = pnp_step(v.z, d.z, alpha); v.w = pnp_step(v.w, d.w, alpha);
        st4(z + r * ldz + c, v);
    }
}

__global__ __launch_bounds__(256) void pnp_update_kernel1(float* __restrict__ z, int ldz, const float* __restrict__ g, int ldg, int64_t M, int C,
                                                          const float* __restrict__ alpha_dev) {
    const float alpha = alpha_dev[0];
    const int64_t total = M * C;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / C;
        const int c = (int)(e - r * C);
        z[r * ldz + c] = pnp_step(z[r * ldz + c], g[r * ldg + c], alpha);
    }
}

static int pnp_grid(int64_t elems) {
    int64_t g = cdiv64(elems, 256);
    const int64_t cap = (int64_t)num_cus() * 16;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}

// Do the channel slices [M rows][C] at a (row pitch lda) and b (row pitch ldb) share an element?  Slices of ONE tensor (equal pitch)
// are told apart by their column windows; everything else by its whole extent.
static bool slices_overlap(const void* a, int64_t lda, const void* b, int64_t ldb, int64_t M, int64_t C) {
    const int64_t pa = (int64_t)reinterpret_cast<uintptr_t>(a), pb = (int64_t)reinterpret_cast<uintptr_t>(b);
    const int64_t ea = ((M - 1) * lda + C) * 4, eb = ((M - 1) * ldb + C) * 4;
    if (pa + ea <= pb || pb + eb <= pa) return false;
    if (lda != ldb) return true;
    const int64_t pitch = lda * 4;
    int64_t d = (pb - pa) % pitch;
    if (d < 0) d += pitch;
    return !(d >= C * 4 && d + C * 4 <= pitch);
}

static bool vec4_ok(int C, const void* p0, int ld0, const void* p1, int ld1, const void* p2, int ld2) {
    return C % 4 == 0 && ld0 % 4 == 0 && ld1 % 4 == 0 && ld2 % 4 == 0 && aligned16(p0) && aligned16(p1) && aligned16(p2);
}

}  // namespace rd
using namespace rd;

extern "C" int rd_act_gate_t(int32_t dtype, const void* dy, int32_t lddy, const void* y, int32_t ldy, void* out, int32_t ldo, int64_t M,
                             int32_t C, int32_t act, void* stream) {
    RD_CHECK_CODE(dy && y && out, RD_EPNP_NULL, "act_gate: null pointer");
    RD_CHECK_CODE(M > 0 && C > 0, RD_EPNP_RANGE, "act_gate: M %lld, C %d", (long long)M, C);
    RD_CHECK_CODE(lddy >= C && ldy >= C && ldo >= C, RD_EPNP_STRIDE, "act_gate: channel stride below the channel count (lddy %d, ldy %d, ldo %d, C %d)",
                  lddy, ldy, ldo, C);
    RD_CHECK_CODE(!slices_overlap(out, ldo, y, ldy, M, C), RD_EPNP_OVERLAP, "act_gate: out overlaps y");
    RD_CHECK_CODE((out == dy && ldo == lddy) || !slices_overlap(out, ldo, dy, lddy, M, C), RD_EPNP_OVERLAP,
                  "act_gate: out overlaps dy without being dy (in place: same pointer, same stride)");
    RD_CHECK_CODE(act == RD_ACT_RELU, RD_EPNP_ACT, "act_gate: activation %d (ReLU only)", act);
    RD_CHECK_CODE(dtype == RD_DTYPE_F32, RD_EPNP_DTYPE, "act_gate: dtype %d (fp32 tensors only)", dtype);
    const float *dyf = static_cast<const float*>(dy), *yf = static_cast<const float*>(y);
    float* of = static_cast<float*>(out);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec4_ok(C, dy, lddy, y, ldy, out, ldo))
        hipLaunchKernelGGL(act_gate_kernel4, dim3(pnp_grid(M * (C / 4))), dim3(256), 0, s, dyf, lddy, yf, ldy, of, ldo, M, C);
    else
        hipLaunchKernelGGL(act_gate_kernel1, dim3(pnp_grid(M * C)), dim3(256), 0, s, dyf, lddy, yf, ldy, of, ldo, M, C);
    RD_CHECK_LAUNCH("act_gate_kernel");
    return RD_OK;
}

extern "C" int rd_pnp_update(float* z, int32_t ldz, const float* g, int32_t ldg, int64_t M, int32_t C, const float* alpha_dev, void* stream) {
    RD_CHECK_CODE(z && g && alpha_dev, RD_EPNP_NULL, "pnp_update: null pointer");
    RD_CHECK_CODE(M > 0 && C > 0, RD_EPNP_RANGE, "pnp_update: M %lld, C %d", (long long)M, C);
    RD_CHECK_CODE(ldz >= C && ldg >= C, RD_EPNP_STRIDE, "pnp_update: channel stride below the channel count (ldz %d, ldg %d, C %d)", ldz, ldg, C);
    RD_CHECK_CODE(!slices_overlap(z, ldz, g, ldg, M, C), RD_EPNP_OVERLAP, "pnp_update: z overlaps g");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec4_ok(C, z, ldz, g, ldg, z, ldz))
        hipLaunchKernelGGL(pnp_update_kernel4, dim3(pnp_grid(M * (C / 4))), dim3(256), 0, s, z, ldz, g, ldg, M, C, alpha_dev);
    else
        hipLaunchKernelGGL(pnp_update_kernel1, dim3(pnp_grid(M * C)), dim3(256), 0, s, z, ldz, g, ldg, M, C, alpha_dev);
    RD_CHECK_LAUNCH("pnp_update_kernel");
    return RD_OK;
}
