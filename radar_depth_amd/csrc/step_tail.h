// What the kernels of the step's tail share (loss_opt.hip, adam.hip): the two grids and the prologue of a clipped optimizer step.
#pragma once
#include "common.h"

namespace rd {

constexpr int RED_BLOCKS = 1024;

// blocks of a reduction pass: a function of n alone (never of the CU count), so every device forms the same partials
static inline int red_grid(int64_t n) {
    int64_t g = cdiv64(n, 256 * 8);
    if (g > RED_BLOCKS) g = RED_BLOCKS;
    return (int)(g < 1 ? 1 : g);
}
// blocks of a grid-stride streaming pass
static inline int ew_grid2(int64_t n) {
    int64_t g = cdiv64(n, 256);
    const int64_t cap = (int64_t)num_cus() * 16;
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

// ---------------------------------------------------------------- global gradient-norm clip and non-finite guard
// torch.nn.utils.clip_grad_norm_(parameters, c, 2.0) between backward and optimizer.step(), without the norm leaving the device:
// grad_sumsq_kernel leaves one float64 sum of squares per block, every block of the optimizer launch that follows adds those
// (<= RED_BLOCKS words, as the second BerHu pass takes its maxima) and forms the coefficient itself.  No atomics; every order is fixed by n
// alone: a thread's elements in grid-stride order, the lanes' tree (wave_total_lane63), the four waves in order, the partials in
// thread-stride order and the same tree again.  So the partials, the norm and the coefficient are bit-reproducible from call to call
// and equal on every rank of a data-parallel step.
struct ClipArgs {
    double max_norm;
    int skip_nonfinite;
    const double* part;         // n_part sums of squares (rd_grad_sumsq)
    int n_part;
    double* stats;              // [4]: total_norm, coefficient, number of skipped steps, 1.0 if this step is skipped
};
struct ClipDecision {
    float coef;
    bool skip;                  // (block-uniform)
};
// Called by every thread of a 256-thread block (sh: 4 doubles); thread 0 of block 0 writes the stats.  Every operation is rounded on its
// own: the product gscale * sqrt(S) is stats[0] and is not fused into the + 1e-6 that follows, whatever the including file's contraction.
__device__ __forceinline__ ClipDecision clip_prologue(float gscale, const ClipArgs& c, double* sh) {
#pragma clang fp contract(off)
    double a = 0.0;
    for (int i = threadIdx.x; i < c.n_part; i += blockDim.x) a += c.part[i];
    const double S = block_total_d(a, sh);
    const double total_norm = (double)gscale * sqrt(S);
    const double r = c.max_norm / (total_norm + 1e-6);
    ClipDecision d;
    d.coef = c.max_norm > 0.0 ? (float)(r > 1.0 ? 1.0 : r) : 1.f;             // torch.clamp(max=1): a NaN stays a NaN
    d.skip = c.skip_nonfinite && !isfinite(S);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        c.stats[0] = total_norm;
        c.stats[1] = (double)d.coef;
        if (d.skip) c.stats[2] += 1.0;
        c.stats[3] = d.skip ? 1.0 : 0.0;
    }
    return d;
}

}  // namespace rd
