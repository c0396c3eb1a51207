// Early ray termination carried through the OUTSIDE-sphere march of the NeO-360 frame (neo_tp_render_marching with `outside`;
// include/neo360_hip.h: OUTSIDE STOP RULE): a surviving ray's background march stops at the first SEGMENT boundary at which
// bg_lambda x (the background's own transmittance) has fallen below eps.  This file holds everything but the driver
// (tp_eval_outside, api_tp.hip).  The five steps are terminate.hip's, on the COMPACT background rows of the culled frame - row k
// belongs to ray map[k], the survivor count is a device word, the level-0 positions are one shared row:
//
//   k_tout_init      per level: lam_c[k] = the level's lambda of ray map[k], alive 1, stop 0 - and dead rows behind the count;
//   k_tout_emit      the point rows of one segment of the ALIVE rows of one window (launch_cull_compact on the running value);
//                    a row carries its ray's origin, direction and far, the sample's s = 1/r and the view direction of the
//                    quirk-Q1 ray of the DENSE launch of the level's full N, c0 + ((ray - c0) N + j) mod bc on the dense ray index;
//   (scatter)        launch_term_scatter of terminate.hip into the zero-filled compact rows, dst = k N + j;
//   k_tout_advance   the OUTSIDE STOP RULE: one wave per alive row continues k_composite MODE 2's fp64 product and forms the
//                    running value lam_c x (float)carry - one fp32 multiply;
//   k_tout_by_slot   stop / value back behind their rays, 0 for a ray without a slot.
//
// No atomics, no spinning: every count is a device word written by one thread behind its producers in stream order.  The evaluator
// sources are not touched: a point row is evaluated by the compact launch with N = 1 and the identity map, whose point_setup_row
// reads far[row] - hence the far column of OccRows.
#include "common.h"
#include "tp_frame.h"

using namespace neo_host;

namespace neo {

namespace {

constexpr int TOUT_ROWS_PER_BLOCK = 4;      // 4 waves of 64, one compact row each (as k_composite)

__global__ void k_tout_init(const float* __restrict__ lam, const int* __restrict__ map, const int* __restrict__ count, int R,
                            float* __restrict__ lam_c, float* __restrict__ alive, float* __restrict__ value, int* __restrict__ stop,
                            int stop_value, long long* __restrict__ kept, long long kept_per_row) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = *count;
    if (k < R) {
        const bool live = k < n;
        if (lam_c) lam_c[k] = live ? lam[map[k]] : 0.0f;
        if (alive) alive[k] = live ? 1.0f : -1.0f;      // -1 < eps for every eps >= 0: a row behind the count never marches
        if (value) value[k] = 0.0f;
        stop[k] = live ? stop_value : 0;
    }
    if (k == 0 && kept) *kept = kept_per_row * (long long)n;
}

// One window (compact rows k0 .. of the frame's R), one segment (samples b0 .. b0 + len - 1 of the level's N): point row kk len + jj
// is sample b0 + jj of compact row k = k0 + map_w[kk], kk < *count_w.  Thread 0 writes the row count and adds it to *kept_sum
// (behind the previous segment in stream order: no atomic).
__global__ __launch_bounds__(256) void k_tout_emit(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                   const float* __restrict__ viewdirs, const float* __restrict__ far,
                                                   const float* __restrict__ s_rows, long s_stride, const int* __restrict__ map,
                                                   const int* __restrict__ map_w, const int* __restrict__ count_w, int k0, int R,
                                                   int N, int b0, int len, int chunk, float* __restrict__ c_o,
                                                   float* __restrict__ c_d, float* __restrict__ c_v, float* __restrict__ c_t,
                                                   float* __restrict__ c_far, int* __restrict__ dst, int* __restrict__ rows,
                                                   long long* __restrict__ kept_sum) {
    const int alive = *count_w;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p == 0) {
        *rows = alive * len;
        if (kept_sum) *kept_sum = *kept_sum + (long long)alive * len;
    }
    if (p >= (long)alive * len) return;
    const int kk = (int)(p / len), j = b0 + (int)(p - (long)kk * len);
    const int k = k0 + map_w[kk];
    const int ray = map[k];
    const int c0 = (ray / chunk) * chunk;
    const int bc = min(chunk, R - c0);
    const int dray = c0 + (int)(((long)(ray - c0) * N + j) % bc);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c_o[p * 3 + a] = rays_o[(long)ray * 3 + a];
        c_d[p * 3 + a] = rays_d[(long)ray * 3 + a];
        c_v[p * 3 + a] = viewdirs[(long)dray * 3 + a];
    }
    c_t[p] = s_rows[(long)k * s_stride + j];
    c_far[p] = far[ray];
    dst[p] = k * N + j;
}

// OUTSIDE STOP RULE.  Compact row k0 + map_w[kk] (map_w null: row kk; count_w null: n_rows of them), samples b0 .. b_end - 1 of its
// N in segments of `segment` (b0 a multiple of `segment`, so every 64-sample round below is a round of k_composite).  The lines that
// form `keep`, the inclusive fp64 product scan and `carry *=` are k_composite's (sampling.hip) in MODE 2 - delta = s_i - s_{i+1}, the
// last one 1e10, no |d| factor - so that (float)carry at a boundary is the background transmittance that composite assigns to the
// boundary's sample, bit for bit.  After every segment: stop = its end, value = lam_c (float)carry (one fp32 multiply); the march
// over further segments goes on iff !(value < eps) - the negation, so a NaN keeps marching.
__global__ __launch_bounds__(256) void k_tout_advance(const float4* __restrict__ rgbsigma, const float* __restrict__ s_rows,
                                                      long s_stride, int N, int b0, int b_end, int segment, float eps,
                                                      const int* __restrict__ map_w, const int* __restrict__ count_w, int n_rows,
                                                      int k0, const float* __restrict__ lam_c, double* __restrict__ carry_io,
                                                      float* __restrict__ value, float* __restrict__ alive,
                                                      int* __restrict__ stop) {
    const int kk = blockIdx.x * TOUT_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (kk >= (count_w ? *count_w : n_rows)) return;
    const int k = k0 + (map_w ? map_w[kk] : kk);
    const int lane = lane_id();
    const float* tr = s_rows + (long)k * s_stride;
    const float4* cs = rgbsigma + (long)k * N;
    const float lam = lam_c[k];
    double carry = b0 > 0 ? carry_io[k] : 1.0;      // product of (1-alpha+eps) over all earlier samples
    int st = b0;
    float v = lam * (float)carry;
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
                    delta = ti - tn;
                } else {
                    delta = 1e10f;
                }
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
        v = lam * (float)carry;
        sb = e;
        if (e < N && v < eps) break;
    }
    if (lane == 0) {
        stop[k] = st;
        value[k] = v;
        if (alive) alive[k] = v;
        if (carry_io) carry_io[k] = carry;
    }
}

__global__ void k_tout_by_slot(const int* __restrict__ stop_c, const float* __restrict__ value_c, const int* __restrict__ slot, int R,
                               int* __restrict__ stop, float* __restrict__ value) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int k = slot[r];
    if (stop) stop[r] = k >= 0 ? stop_c[k] : 0;
    if (value) value[r] = k >= 0 ? value_c[k] : 0.0f;
}

}  // namespace

void launch_tout_init(const float* lam, const int* map, const int* count, int R, float* lam_c, float* alive, float* value, int* stop,
                      int stop_value, long long* kept, long long kept_per_row, hipStream_t s) {
    if (R > 0)
        hipLaunchKernelGGL(k_tout_init, dim3((R + 255) / 256), dim3(256), 0, s, lam, map, count, R, lam_c, alive, value, stop, stop_value,
                           kept, kept_per_row);
}

void launch_tout_emit(const float* rays_o, const float* rays_d, const float* viewdirs, const float* far, const float* s_rows,
                      long s_stride, const int* map, const int* map_w, const int* count_w, int k0, int rows, int R, int N, int b0, int len,
                      int chunk, const OccRows& w, long long* kept_sum, hipStream_t s) {
    const long P = (long)rows * len;
    if (P <= 0) return;
    hipLaunchKernelGGL(k_tout_emit, dim3((int)((P + 255) / 256)), dim3(256), 0, s, rays_o, rays_d, viewdirs, far, s_rows, s_stride, map,
                       map_w, count_w, k0, R, N, b0, len, chunk, w.o, w.d, w.v, w.t, w.far, w.dst, w.count, kept_sum);
}

void launch_tout_advance(const float* rgbsigma, const float* s_rows, long s_stride, int N, int b0, int b_end, int segment, float eps,
                         const int* map_w, const int* count_w, int n_rows, int k0, const float* lam_c, double* carry, float* value,
                         float* alive, int* stop, hipStream_t s) {
    if (n_rows <= 0) return;
    hipLaunchKernelGGL(k_tout_advance, dim3((n_rows + TOUT_ROWS_PER_BLOCK - 1) / TOUT_ROWS_PER_BLOCK), dim3(256), 0, s,
                       (const float4*)rgbsigma, s_rows, s_stride, N, b0, b_end, segment, eps, map_w, count_w, n_rows, k0, lam_c, carry,
                       value, alive, stop);
}

void launch_tout_by_slot(const int* stop_c, const float* value_c, const int* slot, int R, int* stop, float* value, hipStream_t s) {
    if (R > 0 && (stop || value))
        hipLaunchKernelGGL(k_tout_by_slot, dim3((R + 255) / 256), dim3(256), 0, s, stop_c, value_c, slot, R, stop, value);
}

}  // namespace neo

extern "C" {

// the pure function k_tout_advance on caller rows; touches no context-owned memory: no ordering scope (as neo_tp_termination_stops)
int neo_tp_termination_stops_outside(neo_ctx* ctx, const float* rgbsigma, const float* s, const float* bg_lambda, int R, int N,
                                     float eps, int segment, int* stop, float* value, void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0 && N >= 1, "bad shape");
    REQUIRE(static_cast<long>(R) * N <= 2147483647L, "too many points for 32-bit indices");
    REQUIRE(eps >= 0.0f && eps < 1.0f, "eps must lie in [0, 1)");
    REQUIRE(segment >= 64 && segment % 64 == 0, "segment must be a positive multiple of 64");
    if (R == 0) return NEO_OK;
    REQUIRE(rgbsigma && s && bg_lambda && stop && value, "null pointer");
    neo::launch_tout_advance(rgbsigma, s, N, N, 0, N, segment, eps, nullptr, nullptr, R, 0, bg_lambda, nullptr, value, nullptr, stop,
                             static_cast<hipStream_t>(stream));
    return check_launch();
}

}  // extern "C"
