// The per-ray extras of a Mip-NeRF 360 interval histogram (edges, w): opacity, expected distance and distance percentiles - the slot
// the reference's volumetric_rendering leaves open behind `compute_extras` (mipnerf360/helper.py:264-274), built from its own
// integrate_weights (:196-203) and sorted_interp (:207-222) - and the backward of (opacity, expected distance) with respect to w.
// One 64-lane wave per ray, four rays per block, like k_mip_composite (mip_sampling.hip) and the regularisers (mip_losses.hip).
// Inputs and outputs are fp32; every prefix sum, every difference taken from one and every quotient is fp64 (s -> t included), and
// each output entry is rounded once.  No atomics: the summation order is fixed, results repeat bit for bit.
#include "common.h"
#include "kernels.h"

namespace neo {

namespace {

constexpr int RPB = 4;                  // rays (waves) per 256-thread block
constexpr int MAXE = 1024;              // intervals per histogram (a block's knot rows: 4 x 1025 doubles of LDS at most)
constexpr int MAXU = 8;                 // quantiles per call

// inclusive scan over the 64 lanes
__device__ __forceinline__ double wave_scan_add(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// An edge as a metric distance: s_near == 0 (near == far == 0 at the entry point) - the row holds distances already; otherwise
// s_to_t of construct_ray_warps (helper.py:168-172), 1 / (s s_far + (1 - s) s_near).
__device__ __forceinline__ double edge_t(float e, double s_near, double s_far) {
    const double s = (double)e;
    return s_near == 0.0 ? s : 1.0 / (s * s_far + (1.0 - s) * s_near);
}

// acc = sum w_i and num = sum w_i (t_i + t_{i+1}) / 2 of one row, the same on every lane: lane l adds intervals l, l + 64, .. in
// order, then a butterfly over the lanes.  Forward and backward share it, so the backward differentiates the mean the forward gave.
__device__ __forceinline__ void row_sums(const float* er, const float* wr, int n, int lane, double s_near, double s_far, double& acc,
                                         double& num) {
    double a = 0.0, m = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double wi = (double)wr[i];
        a += wi;
        m += wi * ((edge_t(er[i], s_near, s_far) + edge_t(er[i + 1], s_near, s_far)) * 0.5);
    }
    acc = wave_sum_f64(a);
    num = wave_sum_f64(m);
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
//   acc  = sum_i w_i
//   mean = clip(nan_to_num(sum_i w_i (t_i + t_{i+1}) / 2 / acc, nan = inf), t_0, t_n)               (a row without weight: t_n)
//   pct  = sorted_interp(u, integrate_weights(w), t): the knots are xp = [0, min(cumsum(w[:-1]), 1), 1] (n + 1 of them, one per edge,
//          no renormalisation).  Knots and edges do not decrease, so the reference's masked max / min pick the neighbours of the
//          bracket: with c = #{j : xp_j <= u} (>= 1, since xp_0 = 0 <= u), (xp0, fp0) = knot / edge c - 1 and (xp1, fp1) = knot / edge
//          min(c, n); offset = clip(nan_to_num((u - xp0) / (xp1 - xp0), 0), 0, 1), result fp0 + offset (fp1 - fp0).
// The row is walked in rounds of 64 with a shuffle scan and a carried prefix; each round adds its knots <= u_q to c_q by ballot and
// popcount and leaves the knots in the wave's LDS row, from which lane q interpolates quantile q afterwards.
// Surplus waves of the last block redo the last ray and write nothing: the barrier stays uniform (as k_mip_outer).
__global__ __launch_bounds__(256) void k_mip_extras(const float* __restrict__ edges, const float* __restrict__ w, int R, int n,
                                                     double s_near, double s_far, const float* __restrict__ u, int n_u,
                                                     float* __restrict__ acc_out, float* __restrict__ mean_out,
                                                     float* __restrict__ pct_out) {
    extern __shared__ double s_c[];                          // RPB rows of n + 1 knots
    const int wv = threadIdx.x >> 6, lane = lane_id();
    const int ray_raw = blockIdx.x * RPB + wv;
    const bool live = ray_raw < R;
    const int ray = live ? ray_raw : R - 1;
    const float* er = edges + (long)ray * (n + 1);
    const float* wr = w + (long)ray * n;
    if (acc_out || mean_out) {                               // uniform over the grid
        double acc, num;
        row_sums(er, wr, n, lane, s_near, s_far, acc, num);
        if (live && lane == 0) {
            if (acc_out) acc_out[ray] = (float)acc;
            if (mean_out) {
                double m = num / acc;
                if (m != m) m = __builtin_inf();
                mean_out[ray] = (float)fmin(fmax(m, edge_t(er[0], s_near, s_far)), edge_t(er[n], s_near, s_far));
            }
        }
    }
    if (pct_out == nullptr || n_u == 0) return;              // uniform over the grid
    double* C = s_c + wv * (n + 1);
    float uq[MAXU];
    int cnt[MAXU];
#pragma unroll
    for (int q = 0; q < MAXU; ++q) {
        uq[q] = q < n_u ? u[q] : 0.0f;
        cnt[q] = ((double)uq[q] >= 0.0 ? 1 : 0) + ((double)uq[q] >= 1.0 ? 1 : 0);      // the end knots 0 and 1
    }
    double carry = 0.0;
    for (int base = 0; base < n - 1; base += 64) {           // knot i + 1 = min(w_0 + .. + w_i, 1) for i < n - 1
        const int i = base + lane;
        const bool valid = i < n - 1;
        const double incl = wave_scan_add(valid ? (double)wr[i] : 0.0, lane);
        const double knot = fmin(carry + incl, 1.0);
        if (valid) C[i + 1] = knot;
        carry += __shfl(incl, 63, 64);
#pragma unroll
        for (int q = 0; q < MAXU; ++q)
            if (q < n_u) cnt[q] += __popcll(__ballot(valid && (double)uq[q] >= knot));
    }
    if (lane == 0) { C[0] = 0.0; C[n] = 1.0; }
    __syncthreads();
    int c = 0;
    float uv = 0.0f;
#pragma unroll
    for (int q = 0; q < MAXU; ++q)
        if (lane == q) { c = cnt[q]; uv = uq[q]; }
    if (live && lane < n_u && c >= 1) {                      // c == 0: a quantile below 0 or a NaN, outside the contract - nothing written
        const int j0 = c - 1, j1 = c < n ? c : n;
        const double xp0 = C[j0], xp1 = C[j1];
        const double fp0 = edge_t(er[j0], s_near, s_far), fp1 = edge_t(er[j1], s_near, s_far);
        double off = ((double)uv - xp0) / (xp1 - xp0);
        if (off != off) off = 0.0;
        off = fmin(fmax(off, 0.0), 1.0);
        pct_out[(long)ray * n_u + lane] = (float)(fp0 + off * (fp1 - fp0));
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// g_w_i = g_acc + g_mean ((t_i + t_{i+1}) / 2 - mean) / acc with mean = num / acc before the clip (the mean of midpoints lies inside
// [t_0, t_n]; the clip only catches the row without weight).  On a row with acc == 0 the second term is DEFINED as 0 (autograd of
// the forward's expression yields NaN there).  A NULL upstream pointer stands for zeros.
__global__ __launch_bounds__(256) void k_mip_extras_bwd(const float* __restrict__ edges, const float* __restrict__ w, int R, int n,
                                                         double s_near, double s_far, const float* __restrict__ g_acc,
                                                         const float* __restrict__ g_mean, float* __restrict__ g_w) {
    const int lane = lane_id();
    const int ray = blockIdx.x * RPB + (threadIdx.x >> 6);
    if (ray >= R) return;
    const float* er = edges + (long)ray * (n + 1);
    const float* wr = w + (long)ray * n;
    const double ga = g_acc ? (double)g_acc[ray] : 0.0;
    double scale = 0.0, mean = 0.0;
    if (g_mean) {                                            // uniform over the grid
        double acc, num;
        row_sums(er, wr, n, lane, s_near, s_far, acc, num);
        if (acc != 0.0) {
            scale = (double)g_mean[ray] / acc;
            mean = num / acc;
        }
    }
    for (int i = lane; i < n; i += 64) {
        const double mid = (edge_t(er[i], s_near, s_far) + edge_t(er[i + 1], s_near, s_far)) * 0.5;
        g_w[(long)ray * n + i] = (float)(ga + scale * (mid - mean));
    }
}

// near == far == 0: metric edges; otherwise s_near = 1 / near, s_far = 1 / far as the reference's python floats
inline void warp_of(float near, float far, double& s_near, double& s_far) {
    s_near = near == 0.0f ? 0.0 : 1.0 / static_cast<double>(near);
    s_far = far == 0.0f ? 0.0 : 1.0 / static_cast<double>(far);
}

}  // namespace

int launch_mip_extras(const float* edges, const float* w, int R, int n, float near, float far, const float* u, int n_u, float* acc,
                      float* dist_mean, float* dist_pct, hipStream_t s) {
    if (n < 1 || n > MAXE || n_u < 0 || n_u > MAXU || (near == 0.0f) != (far == 0.0f)) return -1;
    if (R <= 0) return 0;
    double s_near, s_far;
    warp_of(near, far, s_near, s_far);
    const size_t lds = dist_pct && n_u ? sizeof(double) * RPB * (n + 1) : 0;
    hipLaunchKernelGGL(k_mip_extras, dim3((R + RPB - 1) / RPB), dim3(256), lds, s, edges, w, R, n, s_near, s_far, u, n_u, acc, dist_mean,
                       dist_pct);
    return 0;
}

int launch_mip_extras_bwd(const float* edges, const float* w, int R, int n, float near, float far, const float* g_acc,
                          const float* g_mean, float* g_w, hipStream_t s) {
    if (n < 1 || n > MAXE || (near == 0.0f) != (far == 0.0f)) return -1;
    if (R <= 0) return 0;
    double s_near, s_far;
    warp_of(near, far, s_near, s_far);
    hipLaunchKernelGGL(k_mip_extras_bwd, dim3((R + RPB - 1) / RPB), dim3(256), 0, s, edges, w, R, n, s_near, s_far, g_acc, g_mean, g_w);
    return 0;
}

}  // namespace neo
