// The geometry of transform_train's depth chain, shared by staging_train.hip (depth planes) and radar_filter.hip (index_map): the
// per-chunk frame records, scipy.ndimage's order-0 rotation sample and the clamped NEAREST table lookup.  Contraction stays off from
// here to the end of the including file: the rotation coordinates must round like the reference's separate multiplies and adds.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace rd {

constexpr int kChunk = RD_STAGE_TRAIN_CHUNK;
struct TrainFrames { RdStageTrainFrame f[kChunk]; };

// scipy.ndimage's order-0 sample of output pixel (y, x) of the rotation: the source index, or false where the reference writes cval = 0
__device__ __forceinline__ bool rot_src(const double m00, const double m01, const double off0, const double m10, const double m11, const double off1,
                                        int H0, int W0, int y, int x, int& iy, int& ix) {
    const double fy = (double)y, fx = (double)x;
    const double cy = (fy * m00 + fx * m01) + off0;
    const double cx = (fy * m10 + fx * m11) + off1;
    const bool ok = cy >= 0.0 && cy <= (double)(H0 - 1) && cx >= 0.0 && cx <= (double)(W0 - 1);      // false for NaN as well
    iy = ok ? (int)floor(cy + 0.5) : 0;
    ix = ok ? (int)floor(cx + 0.5) : 0;
    return ok;
}

// entry i of frame b's NEAREST table ([B, n]), clamped to the frame: a wrong table gives wrong pixels, never an out-of-bounds read
__device__ __forceinline__ int near_src(const int32_t* __restrict__ near, int b, int n, int i, int size) {
    return min(max(near[(int64_t)b * n + i], 0), size - 1);
}

}  // namespace rd
