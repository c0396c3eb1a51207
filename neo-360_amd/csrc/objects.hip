// Object-level render of NeRF_TP (neo_tp_render_objects): the two inside-sphere MLPs are marched between a caller-given per-ray
// interval [near_obj, far_obj] - the output of neo_aabb_multi / ops.sample_rays_in_bbox - for the rays that have one.
//
// Hit rule: lo = max(near_obj, 1e-4) (the reference's near, neo360/model.py:277; also for an origin inside a box, where the slab
// test gives tmin <= 0), hi = far_obj; a ray is a HIT iff both bounds are finite and hi > lo.  It is written as the negation of
// the failing comparisons, so a NaN bound makes the ray a miss; the reference's "0 = no hit" sentinel falls out of the rule.
//
// This file holds the stable compaction of the hit rays (the two-launch scheme of compact.h: no atomics, the same map on every
// run, the count stays on the device), the level-0 rows of the compact rays, and the scatter that puts compact results back
// behind their rays.  Everything between them - evaluators, compositing, resampling - is the existing kernels on compact rows.
#include "common.h"
#include "compact.h"
#include "kernels.h"

namespace neo {

namespace {

constexpr int OBJ_BLOCK = compact::BLOCK;
constexpr float OBJ_NEAR = 1e-4f;          // neo360/model.py:277

__device__ __forceinline__ float obj_lo(float near) { return near > OBJ_NEAR ? near : OBJ_NEAR; }

// the negation of the failing comparisons: a NaN (or infinite) bound fails `< inf`, a NaN far fails `>`
__device__ __forceinline__ bool obj_hit(const float* __restrict__ near_obj, const float* __restrict__ far_obj, int ray, int R) {
    if (ray >= R) return false;
    const float n = near_obj[ray], f = far_obj[ray];
    return !(!(fabsf(n) < __builtin_inff()) || !(fabsf(f) < __builtin_inff()) || !(f > obj_lo(n)));
}

__global__ __launch_bounds__(OBJ_BLOCK) void k_obj_totals(const float* __restrict__ near_obj, const float* __restrict__ far_obj,
                                                          int R, int* __restrict__ totals) {
    __shared__ int s_wave[OBJ_BLOCK / 64];
    compact::totals_body([&](int ray) { return obj_hit(near_obj, far_obj, ray, R); }, s_wave, totals);
}

__global__ __launch_bounds__(OBJ_BLOCK) void k_obj_emit(const float* __restrict__ near_obj, const float* __restrict__ far_obj,
                                                        int R, const int* __restrict__ totals, int* __restrict__ map,
                                                        int* __restrict__ slot, int* __restrict__ count,
                                                        int* __restrict__ count_out) {
    __shared__ int s_part[OBJ_BLOCK / 64];
    __shared__ int s_wave[OBJ_BLOCK / 64];
    compact::emit_body([&](int ray) { return obj_hit(near_obj, far_obj, ray, R); }, R, totals, s_part, s_wave, map, slot, count,
                       count_out);
}

// compact row k = ray map[k]: t0_c[k, i] = lo (1 - e_i) + hi e_i (neo360/helper.py:36-42, the arithmetic of k_tp_level0),
// far_c[k] = hi, rays_d_c[k, :] = rays_d[ray, :] - what k_composite (mode 1) and k_resample read by row
__global__ void k_obj_level0(const float* __restrict__ near_obj, const float* __restrict__ far_obj,
                             const float* __restrict__ rays_d, const float* __restrict__ edges, const int* __restrict__ map,
                             const int* __restrict__ count, int N, float* __restrict__ t0_c, float* __restrict__ far_c,
                             float* __restrict__ rays_d_c) {
    const long total = (long)*count * N;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int k = (int)(idx / N), i = (int)(idx - (long)k * N);
        const int ray = map[k];
        const float e = edges[i];
        const float near = obj_lo(near_obj[ray]), far = far_obj[ray];
        const float lo = near * (1.0f - e);
        const float hi = far * e;
        t0_c[idx] = lo + hi;
        if (i == 0) {
            far_c[k] = far;
#pragma unroll
            for (int a = 0; a < 3; ++a) rays_d_c[k * 3 + a] = rays_d[ray * 3 + a];
        }
    }
}

// one level's results back behind their rays; a missed ray gets rgb = white ? 1 : 0, acc = 0, depth = 0 and a zero sample row
__global__ void k_obj_scatter(const int* __restrict__ slot, int R, int N, const float* __restrict__ rgb_c,
                              const float* __restrict__ acc_c, const float* __restrict__ depth_c, const float* __restrict__ t_c,
                              int white_bkgd, float* __restrict__ rgb, float* __restrict__ acc, float* __restrict__ depth,
                              float* __restrict__ tvals) {
    const int W = tvals ? N : 1;
    const long total = (long)R * W;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int ray = (int)(idx / W), i = (int)(idx - (long)ray * W);
        const int k = slot[ray];
        if (tvals) tvals[idx] = k >= 0 ? t_c[(long)k * N + i] : 0.0f;
        if (i == 0) {
            const float miss = white_bkgd ? 1.0f : 0.0f;
            if (rgb) {
#pragma unroll
                for (int a = 0; a < 3; ++a) rgb[ray * 3 + a] = k >= 0 ? rgb_c[k * 3 + a] : miss;
            }
            if (acc) acc[ray] = k >= 0 ? acc_c[k] : 0.0f;
            if (depth) depth[ray] = k >= 0 ? depth_c[k] : 0.0f;
        }
    }
}

inline int grid_for(long total) {
    long blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

}  // namespace

void launch_obj_compact(const float* near_obj, const float* far_obj, int R, int* ws, int* count_out, hipStream_t s) {
    if (R <= 0) return;
    const int nb = compact::blocks(R);
    int* count = cull_count_of(ws, R);
    int* totals = count + 1;
    hipLaunchKernelGGL(k_obj_totals, dim3(nb), dim3(OBJ_BLOCK), 0, s, near_obj, far_obj, R, totals);
    hipLaunchKernelGGL(k_obj_emit, dim3(nb), dim3(OBJ_BLOCK), 0, s, near_obj, far_obj, R, totals, cull_map_of(ws, R),
                       cull_slot_of(ws, R), count, count_out);
}

void launch_obj_level0(const float* near_obj, const float* far_obj, const float* rays_d, const float* edges, const int* map,
                       const int* count, int R, int N, float* t0_c, float* far_c, float* rays_d_c, hipStream_t s) {
    if (R <= 0) return;
    hipLaunchKernelGGL(k_obj_level0, dim3(grid_for((long)R * N)), dim3(256), 0, s, near_obj, far_obj, rays_d, edges, map, count, N,
                       t0_c, far_c, rays_d_c);
}

void launch_obj_scatter(const int* slot, int R, int N, const float* rgb_c, const float* acc_c, const float* depth_c,
                        const float* t_c, int white_bkgd, float* rgb, float* acc, float* depth, float* tvals, hipStream_t s) {
    if (R <= 0 || !(rgb || acc || depth || tvals)) return;
    hipLaunchKernelGGL(k_obj_scatter, dim3(grid_for((long)R * (tvals ? N : 1))), dim3(256), 0, s, slot, R, N, rgb_c, acc_c,
                       depth_c, t_c, white_bkgd, rgb, acc, depth, tvals);
}

}  // namespace neo
