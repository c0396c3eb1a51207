// The segmented march of a level (the NeO-360 frames neo_tp_render_terminating / _accelerated / _marching and the vanilla frame
// neo_vanilla_render_marching): a row's march stops at the first SEGMENT boundary at which its running value has fallen below eps
// (include/neo360_hip.h: STOP RULE inside the sphere, OUTSIDE STOP RULE outside, composite mode 0 for vanilla).  This file holds
// the kernels around the point list (point_list.hip); the loop that drives them is march_level (march.h, with the table of what
// differs between the users).  A ROW is a dense ray, or outside the sphere a compact background row of the culled frame (row k
// belongs to ray map[k], the survivor count is a device word).
//
//   k_march_init          per level: alive 1, stop 0 (or N for a level that does not follow the rule), outside also lam_c = the
//                         level's lambda of the row's ray - and dead rows behind the count; the kept count;
//   k_march_scatter       compact (rgb, sigma) rows to their place in the zero-filled rows of the level;
//   k_march_advance       the stop rule: one wave per alive row over the segment's rows continues k_composite's own transmittance
//                         product (composite_round.h) from the row's fp64 carry;
//   k_march_by_slot       stop / value of compact rows back behind their rays, 0 for a ray without a slot;
//   k_march_rows_by_slot  the same for whole rows (the bg_s and bg_rows copies of a culled frame).
//
// A segment's work is proportional to the segment: the point list, the evaluator, scatter and advance touch (alive rows) x
// (segment) points, never the whole row.  No atomics, no spinning: every count is a device word written by one thread behind its
// producers in stream order.
#include "common.h"
#include "composite_round.h"
#include "march.h"
#include "tp_frame.h"

using namespace neo_host;

namespace neo {

namespace {

constexpr int MARCH_ROWS_PER_BLOCK = 4;      // 4 waves of 64, one row each (as k_composite)

__global__ void k_march_init(const float* __restrict__ lam, const int* __restrict__ map, const int* __restrict__ count, int R,
                             float* __restrict__ lam_c, float* __restrict__ alive, float* __restrict__ value, int* __restrict__ stop,
                             int stop_value, long long* __restrict__ kept, long long kept_per_row) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = count ? *count : R;
    if (k < R) {
        const bool live = k < n;
        if (lam_c) lam_c[k] = live ? lam[map[k]] : 0.0f;
        if (alive) alive[k] = live ? 1.0f : -1.0f;      // -1 < eps for every eps >= 0: a row behind the count never marches
        if (value) value[k] = 0.0f;
        if (stop) stop[k] = live ? stop_value : 0;
    }
    if (k == 0 && kept) *kept = kept_per_row * (long long)n;
}

__global__ __launch_bounds__(256) void k_march_scatter(const float4* __restrict__ c_out, const int* __restrict__ dst,
                                                       const int* __restrict__ rows, float4* __restrict__ out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p < (long)*rows) out[dst[p]] = c_out[p];
}

// THE STOP RULE of a region.  Row first + map_w[kk] (map_w null: row kk; count_w null: n_rows of them), samples b0 .. b_end - 1 of
// its N in segments of `segment` (b0 a multiple of `segment`, so every 64-sample round below is a round of k_composite: the same
// two functions of composite_round.h, in mode 1 inside and mode 2 outside, so that (float)carry at a boundary is the transmittance
// that the composite assigns to the boundary's sample, bit for bit).  After every segment: stop = its end, v = (float)carry inside,
// lam_c (float)carry - one fp32 multiply - outside; the march over further segments (b_end beyond the first: the pure functions
// below) goes on iff !(v < eps) - the negation, so a NaN keeps marching.  carry_io (may be null when b0 == 0 and nobody continues):
// the row's fp64 carry.  MODE is the composite's: 1 inside the sphere, 2 outside, and 0 for the vanilla renderer (vanilla_march.hip:
// the last delta is 1e10, every delta times |rays_d|, no far and no lambda; rows are rays, and `stride` is 0 for a level whose rays
// share one row of positions).
template <int MODE>
__global__ __launch_bounds__(256) void k_march_advance(const float4* __restrict__ rgbsigma, const float* __restrict__ pos, long stride,
                                                       const float* __restrict__ rays_d, const float* __restrict__ t_far,
                                                       const float* __restrict__ lam_c, int N, int b0, int b_end, int segment,
                                                       float eps, const int* __restrict__ map_w, const int* __restrict__ count_w,
                                                       int n_rows, int first, double* __restrict__ carry_io,
                                                       float* __restrict__ value, float* __restrict__ alive, int* __restrict__ stop) {
    constexpr int mode = MODE;
    constexpr bool OUTSIDE = MODE == 2;
    const int kk = blockIdx.x * MARCH_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (kk >= (count_w ? *count_w : n_rows)) return;
    const int row = first + (map_w ? map_w[kk] : kk);
    const int lane = lane_id();
    const float* tr = pos + (long)row * stride;
    const float4* cs = rgbsigma + (long)row * N;
    float dnorm = 1.0f, far = 0.0f, lam = 1.0f;
    if constexpr (OUTSIDE) {
        lam = lam_c[row];
    } else {
        const float dx = rays_d[row * 3], dy = rays_d[row * 3 + 1], dz = rays_d[row * 3 + 2];
        dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
        if constexpr (MODE == 1) far = t_far[row];
    }
    double carry = b0 > 0 ? carry_io[row] : 1.0;      // product of (1-alpha+eps) over all earlier samples
    const auto running = [&]() { return OUTSIDE ? lam * (float)carry : (float)carry; };
    int st = b0;
    float v = running();
    for (int sb = b0; sb < b_end;) {
        const int e = min(sb + segment, N);
        for (int base = sb; base < e; base += 64) {
            const int i = base + lane;
            const bool valid = i < N;
            float alpha = 0.f;
            if (valid) alpha = composite_alpha(mode, tr, i, N, tr[i], cs[i].w, far, dnorm);
            (void)transmittance_round(alpha, valid, lane, carry);
        }
        st = e;
        v = running();
        sb = e;
        if (e < N && v < eps) break;
    }
    if (lane == 0) {
        stop[row] = st;
        if (value) value[row] = v;
        if (alive) alive[row] = v;
        if (carry_io) carry_io[row] = carry;
    }
}

__global__ void k_march_by_slot(const int* __restrict__ stop_c, const float* __restrict__ value_c, const int* __restrict__ slot, int R,
                                int* __restrict__ stop, float* __restrict__ value) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int k = slot[r];
    if (stop) stop[r] = k >= 0 ? stop_c[k] : 0;
    if (value) value[r] = k >= 0 ? value_c[k] : 0.0f;
}

__global__ void k_march_rows_by_slot(const float* __restrict__ src_c, const int* __restrict__ slot, long total, int N,
                                     float* __restrict__ dst) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long r = idx / N;
    const int k = slot[r];
    dst[idx] = k >= 0 ? src_c[(long)k * N + (idx - r * N)] : 0.0f;
}

}  // namespace

void launch_march_init(const float* lam, const int* map, const int* count, int R, float* lam_c, float* alive, float* value, int* stop,
                       int stop_value, long long* kept, long long kept_per_row, hipStream_t s) {
    if (R > 0)
        hipLaunchKernelGGL(k_march_init, dim3((R + 255) / 256), dim3(256), 0, s, lam, map, count, R, lam_c, alive, value, stop, stop_value,
                           kept, kept_per_row);
}

void launch_march_scatter(const OccRows& w, long P, float* out, hipStream_t s) {
    if (P <= 0) return;
    hipLaunchKernelGGL(k_march_scatter, dim3((int)((P + 255) / 256)), dim3(256), 0, s, (const float4*)w.out, (const int*)w.dst,
                       (const int*)w.count, (float4*)out);
}

void launch_march_advance(int mode, const float* rgbsigma, const float* pos, long stride, const float* rays_d, const float* t_far,
                          const float* lam_c, int N, int b0, int b_end, int segment, float eps, const int* map_w, const int* count_w,
                          int n_rows, int first, double* carry, float* value, float* alive, int* stop, hipStream_t s) {
    if (n_rows <= 0) return;
    hipLaunchKernelGGL(mode == 2 ? k_march_advance<2> : mode == 1 ? k_march_advance<1> : k_march_advance<0>,
                       dim3((n_rows + MARCH_ROWS_PER_BLOCK - 1) / MARCH_ROWS_PER_BLOCK), dim3(256), 0, s, (const float4*)rgbsigma, pos,
                       stride, rays_d, t_far, lam_c, N, b0, b_end, segment, eps, map_w, count_w, n_rows, first, carry, value, alive, stop);
}

void launch_march_by_slot(const int* stop_c, const float* value_c, const int* slot, int R, int* stop, float* value, hipStream_t s) {
    if (R > 0 && (stop || value))
        hipLaunchKernelGGL(k_march_by_slot, dim3((R + 255) / 256), dim3(256), 0, s, stop_c, value_c, slot, R, stop, value);
}

void launch_march_rows_by_slot(const float* src_c, const int* slot, int R, int N, float* dst, hipStream_t s) {
    const long total = (long)R * N;
    if (total <= 0) return;
    hipLaunchKernelGGL(k_march_rows_by_slot, dim3((int)((total + 255) / 256)), dim3(256), 0, s, src_c, slot, total, N, dst);
}

}  // namespace neo

namespace {

// the pure function k_march_advance on caller rows (ptrs: the entry point has all of its own pointers); touches no context-owned
// memory: no ordering scope (as neo_tp_occupancy_keep)
int march_stops(neo_ctx* ctx, int mode, bool ptrs, const float* rgbsigma, const float* pos, const float* rays_d, const float* t_far,
                const float* lam, int R, int N, float eps, int segment, int* stop, float* value, void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0 && N >= 1, "bad shape");
    REQUIRE(static_cast<long>(R) * N <= 2147483647L, "too many points for 32-bit indices");
    REQUIRE(eps >= 0.0f && eps < 1.0f, "eps must lie in [0, 1)");
    REQUIRE(segment >= 64 && segment % 64 == 0, "segment must be a positive multiple of 64");
    if (R == 0) return NEO_OK;
    REQUIRE(ptrs, "null pointer");
    neo::launch_march_advance(mode, rgbsigma, pos, N, rays_d, t_far, lam, N, 0, N, segment, eps, nullptr, nullptr, R, 0, nullptr, value,
                              nullptr, stop, static_cast<hipStream_t>(stream));
    return check_launch();
}

}  // namespace

extern "C" {

int neo_tp_termination_stops(neo_ctx* ctx, const float* rgbsigma, const float* t, const float* rays_d, const float* t_far, int R, int N,
                             float eps, int segment, int* stop, float* trans, void* stream) {
    return march_stops(ctx, 1, rgbsigma && t && rays_d && t_far && stop && trans, rgbsigma, t, rays_d, t_far, nullptr, R, N, eps,
                       segment, stop, trans, stream);
}

int neo_vanilla_termination_stops(neo_ctx* ctx, const float* rgbsigma, const float* t, const float* rays_d, int R, int N, float eps,
                                  int segment, int* stop, float* trans, void* stream) {
    return march_stops(ctx, 0, rgbsigma && t && rays_d && stop && trans, rgbsigma, t, rays_d, nullptr, nullptr, R, N, eps, segment, stop,
                       trans, stream);
}

int neo_tp_termination_stops_outside(neo_ctx* ctx, const float* rgbsigma, const float* s, const float* bg_lambda, int R, int N,
                                     float eps, int segment, int* stop, float* value, void* stream) {
    return march_stops(ctx, 2, rgbsigma && s && bg_lambda && stop && value, rgbsigma, s, nullptr, nullptr, bg_lambda, R, N, eps,
                       segment, stop, value, stream);
}

}  // extern "C"
