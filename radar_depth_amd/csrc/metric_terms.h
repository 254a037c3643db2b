// The per-pixel terms of the evaluation metrics (evaluation/metrics.py:34-58), shared by every kernel that forms these sums
// (loss_opt.hip, metrics_multidist.hip).
#pragma once
#include "common.h"

namespace rd {

// [10]: count, sum d^2, sum |d|, sum |log10 o - log10 t|, sum |d|/t, #(r<1.25), #(r<1.25^2), #(r<1.25^3),
// sum (1/o-1/t)^2, sum |1/o-1/t|   over pixels with t > 0, d = o - t, r = max(o/t, t/o)
// the ten fp32 terms of one valid pixel (t > 0), added in fp64 -- ONE definition for every kernel that produces these sums
__device__ __forceinline__ void metric_terms(float o, float t, double* acc) {
    const float inv_ln10 = 0.4342944819032518f;
    const float ad = fabsf(o - t);
    acc[0] += 1.0;
    acc[1] += (double)(ad * ad);
    acc[2] += (double)ad;
    acc[3] += (double)fabsf(logf(o) * inv_ln10 - logf(t) * inv_ln10);
    acc[4] += (double)(ad / t);
    const float r = fmaxf(o / t, t / o);
    if (r < 1.25f) acc[5] += 1.0;
    if (r < 1.25f * 1.25f) acc[6] += 1.0;
    if (r < 1.25f * 1.25f * 1.25f) acc[7] += 1.0;
    const float id = fabsf(1.f / o - 1.f / t);
    acc[8] += (double)(id * id);
    acc[9] += (double)id;
}

// Metric k (0..9, the argument order of Result.update: irmse, imae, mse, rmse, mae, absrel, lg10, delta1..3) of one row of ten sums,
// as Result.evaluate finalises it.  A row without a valid pixel (count 0) gives 0/0 = NaN in all ten, like the mean of an empty selection.
__device__ __forceinline__ double meter_metric(const double* __restrict__ row, int k) {
    const double c = row[0];
    switch (k) {
        case 0: return sqrt(row[8] / c);
        case 1: return row[9] / c;
        case 2: return row[1] / c;
        case 3: return sqrt(row[1] / c);
        case 4: return row[2] / c;
        case 5: return row[4] / c;
        case 6: return row[3] / c;
        default: return row[k - 2] / c;       // delta1..3 = row[5..7]
    }
}

}  // namespace rd
