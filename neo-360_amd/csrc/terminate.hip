// Early ray termination of the NeO-360 frame (neo_tp_render_terminating): a ray's inside-sphere march stops at the first SEGMENT
// boundary at which its transmittance has fallen below eps.  This file holds everything but the driver (tp_eval_terminating,
// api_tp.hip):
//
//   k_term_init         per level: running transmittance 1, stop 0 (or N for a level that does not follow the rule), the kept count;
//   k_term_emit         the point rows of one segment of the ALIVE rays of one window (the alive rays come from launch_cull_compact
//                       on the running transmittance: ascending ray order, the count in a device word);
//   k_term_scatter      compact (rgb, sigma) rows to their dense place (the dense rows were zero-filled once per level);
//   k_term_advance      the STOP RULE (include/neo360_hip.h): one wave per alive ray over the segment's dense rows, k_composite's
//                       own transmittance product continued from the ray's fp64 carry;
//   k_term_rows_by_slot compact rows back behind their rays, zeros for a ray without a slot (the bg_s copy of a culled frame).
//
// A segment's work is proportional to the segment: emit, the evaluator, scatter and advance touch (alive rays) x (segment) points,
// never the whole row.  No atomics, no spinning: every count is a device word written by one thread behind its producers in stream
// order.  A compact row is ONE point, as in occupancy.hip: the evaluator's compact launch with N = 1 and the identity map takes the
// view direction of row `row` itself, so emit writes the view direction of the quirk-Q1 ray of the DENSE launch of the level's full
// N, c0 + ((r - c0) N + j) mod bc (k_occ_emit's expression).  The evaluator sources are not touched.
#include "common.h"
#include "tp_frame.h"

using namespace neo_host;

namespace neo {

namespace {

constexpr int TERM_RAYS_PER_BLOCK = 4;      // 4 waves of 64, one ray each (as k_composite)

__global__ void k_term_init(float* __restrict__ trans, int* __restrict__ stop, int R, int stop_value, long long* __restrict__ kept,
                            long long kept_value) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) {
        if (trans) trans[r] = 1.0f;
        stop[r] = stop_value;
    }
    if (r == 0 && kept) *kept = kept_value;
}

// One window (rays r0 .. of the frame's R), one segment (samples b0 .. b0 + len - 1 of the level's N): row k len + jj is sample
// b0 + jj of ray r0 + map[k], k < *count.  t: the level's dense (R,N) rows.  dst = the point's index in the dense rows.  Thread 0
// writes the row count and adds it to *kept_sum (behind the previous segment in stream order: no atomic).
__global__ __launch_bounds__(256) void k_term_emit(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                   const float* __restrict__ viewdirs, const float* __restrict__ t,
                                                   const int* __restrict__ map, const int* __restrict__ count, int r0, int R, int N,
                                                   int b0, int len, int chunk, float* __restrict__ c_o, float* __restrict__ c_d,
                                                   float* __restrict__ c_v, float* __restrict__ c_t, int* __restrict__ dst,
                                                   int* __restrict__ rows, long long* __restrict__ kept_sum) {
    const int alive = *count;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p == 0) {
        *rows = alive * len;
        if (kept_sum) *kept_sum = *kept_sum + (long long)alive * len;
    }
    if (p >= (long)alive * len) return;
    const int k = (int)(p / len), j = b0 + (int)(p - (long)k * len);
    const int ray = r0 + map[k];
    const int c0 = (ray / chunk) * chunk;
    const int bc = min(chunk, R - c0);
    const int dray = c0 + (int)(((long)(ray - c0) * N + j) % bc);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c_o[p * 3 + a] = rays_o[(long)ray * 3 + a];
        c_d[p * 3 + a] = rays_d[(long)ray * 3 + a];
        c_v[p * 3 + a] = viewdirs[(long)dray * 3 + a];
    }
    c_t[p] = t[(long)ray * N + j];
    dst[p] = ray * N + j;
}

__global__ __launch_bounds__(256) void k_term_scatter(const float4* __restrict__ c_out, const int* __restrict__ dst,
                                                      const int* __restrict__ rows, float4* __restrict__ out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p < (long)*rows) out[dst[p]] = c_out[p];
}

// STOP RULE.  Ray r0 + map[k] (map null: ray k; count null: n_rays of them), samples b0 .. b_end - 1 of its N in segments of
// `segment` (b0 a multiple of `segment`, so every 64-sample round below is a round of k_composite).  The lines that form `keep`,
// the inclusive fp64 product scan and `carry *=` are k_composite's (sampling.hip, mode 1), so that (float)carry at a boundary is
// the transmittance that composite assigns to the boundary's sample, bit for bit.  After every segment: stop = its end, trans =
// (float)carry; the march over further segments (b_end beyond the first: neo_tp_termination_stops) goes on iff !(trans < eps) -
// the negation, so a NaN keeps marching.  carry_io (may be null when b0 == 0 and nobody continues): the ray's fp64 carry.
__global__ __launch_bounds__(256) void k_term_advance(const float4* __restrict__ rgbsigma, const float* __restrict__ t,
                                                      const float* __restrict__ rays_d, const float* __restrict__ t_far, int N, int b0,
                                                      int b_end, int segment, float eps, const int* __restrict__ map,
                                                      const int* __restrict__ count, int n_rays, int r0,
                                                      double* __restrict__ carry_io, float* __restrict__ trans,
                                                      int* __restrict__ stop) {
    const int k = blockIdx.x * TERM_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (k >= (count ? *count : n_rays)) return;
    const int ray = r0 + (map ? map[k] : k);
    const int lane = lane_id();
    const float* tr = t + (long)ray * N;
    const float4* cs = rgbsigma + (long)ray * N;
    const float dx = rays_d[ray * 3], dy = rays_d[ray * 3 + 1], dz = rays_d[ray * 3 + 2];
    const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
    const float far = t_far[ray];
    double carry = b0 > 0 ? carry_io[ray] : 1.0;      // product of (1-alpha+eps) over all earlier samples
    int st = b0;
    float tcut = (float)carry;
    for (int sb = b0; sb < b_end;) {
        const int e = min(sb + segment, N);
        for (int base = sb; base < e; base += 64) {
            const int i = base + lane;
            const bool valid = i < N;
            float alpha = 0.f;
            if (valid) {
                const float ti = tr[i];
                const float4 c = cs[i];
                float delta;
                if (i < N - 1) {
                    const float tn = tr[i + 1];
                    delta = tn - ti;
                } else {
                    delta = far - ti;
                }
                delta = delta * dnorm;
                alpha = alpha_of(c.w * delta);
            }
            const float keep = valid ? (1.0f - alpha) + 1e-10f : 1.0f;
            // inclusive product scan in fp64
            double incl = (double)keep;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double up = __shfl_up(incl, o, 64);
                if (lane >= o) incl = up * incl;
            }
            carry = carry * __shfl(incl, 63, 64);
        }
        st = e;
        tcut = (float)carry;
        sb = e;
        if (e < N && tcut < eps) break;
    }
    if (lane == 0) {
        stop[ray] = st;
        trans[ray] = tcut;
        if (carry_io) carry_io[ray] = carry;
    }
}

__global__ void k_term_rows_by_slot(const float* __restrict__ src_c, const int* __restrict__ slot, long total, int N,
                                    float* __restrict__ dst) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long r = idx / N;
    const int k = slot[r];
    dst[idx] = k >= 0 ? src_c[(long)k * N + (idx - r * N)] : 0.0f;
}

}  // namespace

void launch_term_init(float* trans, int* stop, int R, int stop_value, long long* kept, long long kept_value, hipStream_t s) {
    if (R > 0) hipLaunchKernelGGL(k_term_init, dim3((R + 255) / 256), dim3(256), 0, s, trans, stop, R, stop_value, kept, kept_value);
}

void launch_term_emit(const float* rays_o, const float* rays_d, const float* viewdirs, const float* t, const int* map, const int* count,
                      int r0, int rays, int R, int N, int b0, int len, int chunk, const OccRows& w, long long* kept_sum, hipStream_t s) {
    const long P = (long)rays * len;
    if (P <= 0) return;
    hipLaunchKernelGGL(k_term_emit, dim3((int)((P + 255) / 256)), dim3(256), 0, s, rays_o, rays_d, viewdirs, t, map, count, r0, R, N, b0,
                       len, chunk, w.o, w.d, w.v, w.t, w.dst, w.count, kept_sum);
}

void launch_term_scatter(const OccRows& w, long P, float* out, hipStream_t s) {
    if (P <= 0) return;
    hipLaunchKernelGGL(k_term_scatter, dim3((int)((P + 255) / 256)), dim3(256), 0, s, (const float4*)w.out, (const int*)w.dst,
                       (const int*)w.count, (float4*)out);
}

void launch_term_advance(const float* rgbsigma, const float* t, const float* rays_d, const float* t_far, int N, int b0, int b_end,
                         int segment, float eps, const int* map, const int* count, int n_rays, int r0, double* carry, float* trans,
                         int* stop, hipStream_t s) {
    if (n_rays <= 0) return;
    hipLaunchKernelGGL(k_term_advance, dim3((n_rays + TERM_RAYS_PER_BLOCK - 1) / TERM_RAYS_PER_BLOCK), dim3(256), 0, s,
                       (const float4*)rgbsigma, t, rays_d, t_far, N, b0, b_end, segment, eps, map, count, n_rays, r0, carry, trans, stop);
}

void launch_term_rows_by_slot(const float* src_c, const int* slot, int R, int N, float* dst, hipStream_t s) {
    const long total = (long)R * N;
    if (total <= 0) return;
    hipLaunchKernelGGL(k_term_rows_by_slot, dim3((int)((total + 255) / 256)), dim3(256), 0, s, src_c, slot, total, N, dst);
}

}  // namespace neo

extern "C" {

// the pure function k_term_advance on caller rows; touches no context-owned memory: no ordering scope (as neo_tp_occupancy_keep)
int neo_tp_termination_stops(neo_ctx* ctx, const float* rgbsigma, const float* t, const float* rays_d, const float* t_far, int R, int N,
                             float eps, int segment, int* stop, float* trans, void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0 && N >= 1, "bad shape");
    REQUIRE(static_cast<long>(R) * N <= 2147483647L, "too many points for 32-bit indices");
    REQUIRE(eps >= 0.0f && eps < 1.0f, "eps must lie in [0, 1)");
    REQUIRE(segment >= 64 && segment % 64 == 0, "segment must be a positive multiple of 64");
    if (R == 0) return NEO_OK;
    REQUIRE(rgbsigma && t && rays_d && t_far && stop && trans, "null pointer");
    neo::launch_term_advance(rgbsigma, t, rays_d, t_far, N, 0, N, segment, eps, nullptr, nullptr, R, 0, nullptr, trans, stop,
                             static_cast<hipStream_t>(stream));
    return check_launch();
}

}  // extern "C"
