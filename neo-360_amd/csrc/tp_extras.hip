// The per-ray extras of a NeO-360 ray's WHOLE interval histogram, inside and outside the unit sphere together, as distances along
// the ray (the unit of the ray parameter t of o + t d, the unit of the reference's fg_depth): total opacity, expected disparity
// and distance percentiles.  The reference composites comp_depth = fg_depth + bg_lambda * bg_depth (neo360/model.py:523), a
// distance plus a disparity; this is the depth a consumer can use wherever the foreground is not opaque.
// One 64-lane wave per ray, four rays per block, like k_composite (sampling.hip) and k_mip_extras (mip_extras.hip).  Inputs and
// outputs are fp32; everything in between is fp64 and each output entry is rounded once.  No atomics, no LDS, no workgroup
// barrier: the summation order is fixed, results repeat bit for bit, and surplus waves of the last block leave at once.
//
// Histogram, M = 2 N intervals in ray order (N when there are no outside rows):
//   inside  i: [fg_t[i], fg_t[i+1]] with fg_t[N] := far (the sphere exit), mass fg_w[i];
//   outside j: in inverse radius [bg_s[j], bg_s[j+1]] with bg_s[N] := 0 (the reference's 1e10 last step: out to infinite radius),
//              mass lambda * bg_w[j]; the edge at inverse radius s lies at the distance
//              tau(s) = d1 + sqrt(max(1 / s^2 - rho2, 0)) / |d|,  d1 = -(o.d) / |d|^2,  rho2 = |o + d1 d|^2,  tau(0) = +inf
//              (|o + t d| = 1 / s; tau(1) is the sphere exit, so the histogram is continuous there).
// Knots c_0 = 0, c_{k+1} = c_k + m_k, no renormalisation and no clamp.
//   opacity   = c_M
//   disparity = sum_k m_k (1 / a_k + 1 / b_k) / 2 over the interval ends as distances, 1 / inf = 0
//   pct[q]    = +inf when u_q >= c_M (the ray leaves); otherwise with c_k <= u_q < c_{k+1} and off = (u_q - c_k) / m_k:
//               inside a + off (b - a); outside tau(s_j + off (s_{j+1} - s_j)), linear in inverse radius.
#include "common.h"
#include "kernels.h"

namespace neo {

namespace {

constexpr int RPB = 4;                  // rays (waves) per 256-thread block
constexpr int MAXN = 1024;              // samples per region
constexpr int MAXU = 8;                 // quantiles per call

struct RayGeom { double d1, rho2, dn; };

__device__ __forceinline__ double tau_of(double s, const RayGeom& g) {
    if (s == 0.0) return __builtin_inf();
    return g.d1 + sqrt(fmax(1.0 / (s * s) - g.rho2, 0.0)) / g.dn;
}

// One round of 64 intervals of a region: lane `lane` holds interval base + lane with mass m between the knots lo = carry +
// (exclusive prefix) and hi = carry + (inclusive prefix).  lo of lane l + 1 IS hi of lane l and the next round's carry IS hi of
// lane 63, so the brackets [lo, hi) tile [0, c_M) without gap or overlap and a quantile is claimed by one lane of one round.
__device__ __forceinline__ void scan_round(double m, int lane, double& carry, double& lo, double& hi) {
    double incl = m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    double excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.0;
    lo = carry + excl;
    hi = carry + incl;
    carry = __shfl(hi, 63, 64);
}

__global__ __launch_bounds__(256) void k_tp_extras(const float* __restrict__ fg_t, const float* __restrict__ fg_w,
                                                    const float* __restrict__ far, const float* __restrict__ bg_s,
                                                    const float* __restrict__ bg_w, const float* __restrict__ lambda,
                                                    const float* __restrict__ rays_o, const float* __restrict__ rays_d, int R, int N,
                                                    const float* __restrict__ u, int n_u, float* __restrict__ opacity_out,
                                                    float* __restrict__ disparity_out, float* __restrict__ pct_out) {
    const int lane = lane_id();
    const int ray = blockIdx.x * RPB + (threadIdx.x >> 6);
    if (ray >= R) return;                                    // wave-uniform; nothing below synchronises across waves
    RayGeom g;
    {
        const double ox = rays_o[ray * 3L], oy = rays_o[ray * 3L + 1], oz = rays_o[ray * 3L + 2];
        const double dx = rays_d[ray * 3L], dy = rays_d[ray * 3L + 1], dz = rays_d[ray * 3L + 2];
        const double dd = dx * dx + dy * dy + dz * dz;
        g.d1 = -(ox * dx + oy * dy + oz * dz) / dd;
        const double cx = ox + g.d1 * dx, cy = oy + g.d1 * dy, cz = oz + g.d1 * dz;
        g.rho2 = cx * cx + cy * cy + cz * cz;
        g.dn = sqrt(dd);
    }
    if (pct_out == nullptr) n_u = 0;
    double uq[MAXU];
#pragma unroll
    for (int q = 0; q < MAXU; ++q) uq[q] = q < n_u ? (double)u[q] : 0.0;
    unsigned found = 0;                                      // bit q: quantile q has been claimed (the same on every lane)
    double carry = 0.0, disp = 0.0;
    const int regions = bg_s ? 2 : 1;
    for (int region = 0; region < regions; ++region) {
        const float* e = (region == 0 ? fg_t : bg_s) + (long)ray * N;
        const float* w = (region == 0 ? fg_w : bg_w) + (long)ray * N;
        const double scale = region == 0 ? 1.0 : (double)lambda[ray];
        const double e_end = region == 0 ? (double)far[ray] : 0.0;
        for (int base = 0; base < N; base += 64) {
            const int i = base + lane;
            const bool valid = i < N;
            double m = 0.0, e0 = 0.0, e1 = 0.0, a = 0.0, b = 0.0;
            if (valid) {
                m = scale * (double)w[i];
                e0 = (double)e[i];
                e1 = i + 1 < N ? (double)e[i + 1] : e_end;
                a = region == 0 ? e0 : tau_of(e0, g);
                b = region == 0 ? e1 : tau_of(e1, g);
                disp += m * ((1.0 / a + 1.0 / b) * 0.5);
            }
            double lo, hi;
            scan_round(m, lane, carry, lo, hi);
#pragma unroll
            for (int q = 0; q < MAXU; ++q) {
                if (q >= n_u || ((found >> q) & 1u)) continue;
                const unsigned long long hit = __ballot(valid && lo <= uq[q] && uq[q] < hi);
                if (hit == 0ull) continue;
                found |= 1u << q;
                if (lane == __ffsll((long long)hit) - 1) {      // the first claimant: knots of non-negative masses do not decrease
                    // m > 0 in exact arithmetic; a bracket that only the rounding of two prefix sums opened (m == 0) gives its start
                    const double off = m > 0.0 ? fmin((uq[q] - lo) / m, 1.0) : 0.0;
                    const double v = region == 0 ? a + off * (b - a) : tau_of(e0 + off * (e1 - e0), g);
                    pct_out[(long)ray * n_u + q] = (float)v;
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) disp += __shfl_xor(disp, o, 64);
    if (lane == 0) {
        if (opacity_out) opacity_out[ray] = (float)carry;
        if (disparity_out) disparity_out[ray] = (float)disp;
    }
    // unclaimed: u >= c_M, the ray leaves (a NaN or a negative quantile is outside the contract and reads NaN)
    if (lane < n_u && !((found >> lane) & 1u)) {
        double uv = 0.0;
#pragma unroll
        for (int q = 0; q < MAXU; ++q)
            if (lane == q) uv = uq[q];
        pct_out[(long)ray * n_u + lane] = uv >= carry ? __builtin_inff() : __builtin_nanf("");
    }
}

}  // namespace

int launch_tp_extras(const float* fg_t, const float* fg_w, const float* far, const float* bg_s, const float* bg_w, const float* lambda,
                     const float* rays_o, const float* rays_d, int R, int N, const float* u, int n_u, float* opacity, float* disparity,
                     float* dist_pct, hipStream_t s) {
    if (N < 1 || N > MAXN || n_u < 0 || n_u > MAXU) return -1;
    if ((bg_s != nullptr) != (bg_w != nullptr) || (bg_s != nullptr) != (lambda != nullptr)) return -1;
    if (R <= 0 || !(opacity || disparity || (dist_pct && n_u))) return 0;
    hipLaunchKernelGGL(k_tp_extras, dim3((R + RPB - 1) / RPB), dim3(256), 0, s, fg_t, fg_w, far, bg_s, bg_w, lambda, rays_o, rays_d, R, N,
                       u, n_u, opacity, disparity, dist_pct);
    return 0;
}

}  // namespace neo
