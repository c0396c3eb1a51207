// One 64-sample round of the along-ray transmittance product, written once: k_composite (sampling.hip) and the march's stop rules
// (k_march_advance, march.hip) both call these functions and nothing else forms `keep`, so that (float)carry at a segment boundary
// is the transmittance that the composite assigns to the boundary's sample, bit for bit, by construction.
//
//   mode 0: vanilla_nerf/helper.py:521-559   (delta_last 1e10, x|d|)
//   mode 1: neo360/helper.py:128-171 inside  (delta_last = t_far - t_last, x|d|)
//   mode 2: neo360/helper.py:128-171 outside (t descending, delta_i = t_i - t_{i+1}, last 1e10, no |d|)
#pragma once
#include "common.h"

namespace neo {

// alpha of sample i < N of the row tr (ti = tr[i], already loaded by the caller); far is read in mode 1, dnorm = |d| outside mode 2
__device__ __forceinline__ float composite_alpha(int mode, const float* __restrict__ tr, int i, int N, float ti, float sigma, float far,
                                                 float dnorm) {
    float delta;
    if (i < N - 1) {
        const float tn = tr[i + 1];
        delta = mode == 2 ? ti - tn : tn - ti;
    } else {
        delta = mode == 1 ? far - ti : 1e10f;
    }
    if (mode != 2) delta = delta * dnorm;
    return alpha_of(sigma * delta);
}

// The round itself, one sample per lane (alpha = 0 and valid = false behind the row's end).  The inclusive product of
// keep = (1 - alpha) + 1e-10 is scanned in fp64 (the reference's CPU cumprod accumulates in double).  Returns the transmittance in
// front of this lane's sample - carry x the exclusive product, still fp64 - and multiplies carry, the product over all earlier
// samples, by the whole round.
__device__ __forceinline__ double transmittance_round(float alpha, bool valid, int lane, double& carry) {
    const float keep = valid ? (1.0f - alpha) + 1e-10f : 1.0f;
    double incl = (double)keep;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(incl, o, 64);
        if (lane >= o) incl = up * incl;
    }
    double excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 1.0;
    const double front = carry * excl;
    carry = carry * __shfl(incl, 63, 64);
    return front;
}

}  // namespace neo
