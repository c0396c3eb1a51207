// Background culling of the NeO-360 frame render (neo_tp_render_culled): once the foreground of both levels is composited, a
// ray's background can change its colour by < 1.002 bg_lambda and its depth by < 1.001 bg_lambda, so rays whose foreground
// transmittance is below eps at BOTH levels skip the two background evaluations.  This file holds the stable compaction of the
// surviving rays and the merge that puts compact background rows back behind their rays.
//
// Compaction (the scheme of compact.h, shared with objects.hip), two launches over workgroups of 256 rays (4 waves):
//   k_cull_totals : keep mask -> wave ballot + popcount -> one total per workgroup
//   k_cull_emit   : every workgroup sums the totals in front of it (fixed order), recomputes its ballots and writes
//                   map[k] = ray, slot[ray] = k or -1; the last workgroup writes the count
// No atomics and no look-back spinning: survivors come out in ascending ray order, identically on every run (the evaluators'
// results are bitwise repeatable and their quirk-Q1 direction index depends on ray identity, not on the slot).  The count
// stays on the device: the launches that consume compact arrays are sized for all R rays and read it there.
#include "common.h"
#include "compact.h"
#include "kernels.h"

namespace neo {

namespace {

constexpr int CULL_BLOCK = compact::BLOCK;

// the negation of `<`, so that a NaN transmittance survives (and reaches the caller through the un-culled arithmetic)
__device__ __forceinline__ bool cull_keep(const float* __restrict__ lam0, const float* __restrict__ lam1, int ray, int R, float eps) {
    return ray < R && (!(lam0[ray] < eps) || !(lam1[ray] < eps));
}

// the two launches of compact.h with this file's predicate
__global__ __launch_bounds__(CULL_BLOCK) void k_cull_totals(const float* __restrict__ lam0, const float* __restrict__ lam1, int R,
                                                            float eps, int* __restrict__ totals) {
    __shared__ int s_wave[CULL_BLOCK / 64];
    compact::totals_body([&](int ray) { return cull_keep(lam0, lam1, ray, R, eps); }, s_wave, totals);
}

__global__ __launch_bounds__(CULL_BLOCK) void k_cull_emit(const float* __restrict__ lam0, const float* __restrict__ lam1, int R,
                                                          float eps, const int* __restrict__ totals, int* __restrict__ map,
                                                          int* __restrict__ slot, int* __restrict__ count,
                                                          int* __restrict__ count_out) {
    __shared__ int s_part[CULL_BLOCK / 64];
    __shared__ int s_wave[CULL_BLOCK / 64];
    compact::emit_body([&](int ray) { return cull_keep(lam0, lam1, ray, R, eps); }, R, totals, s_part, s_wave, map, slot, count,
                       count_out);
}

__global__ void k_tp_merge_culled(const float* __restrict__ fg_rgb, const float* __restrict__ fg_depth,
                                  const float* __restrict__ lambda, const float* __restrict__ bg_rgb_c,
                                  const float* __restrict__ bg_depth_c, const int* __restrict__ slot, int R,
                                  float* __restrict__ rgb, float* __restrict__ depth, float* __restrict__ bg_rgb) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int k = slot[r];
    if (k >= 0) {            // the arithmetic of k_tp_merge
        const float lam = lambda[r];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float b = bg_rgb_c[k * 3 + a];
            if (rgb) rgb[r * 3 + a] = fg_rgb[r * 3 + a] + lam * b;
            if (bg_rgb) bg_rgb[r * 3 + a] = b;
        }
        if (depth) depth[r] = fg_depth[r] + lam * bg_depth_c[k];
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (rgb) rgb[r * 3 + a] = fg_rgb[r * 3 + a];
            if (bg_rgb) bg_rgb[r * 3 + a] = 0.0f;
        }
        if (depth) depth[r] = fg_depth[r];
    }
}

inline int cull_blocks(int R) { return compact::blocks(R); }

}  // namespace

size_t cull_ws_ints(int R) { return 2 * (size_t)R + 1 + (size_t)cull_blocks(R); }

void launch_cull_compact(const float* lam0, const float* lam1, int R, float eps, int* ws, int* count_out, hipStream_t s) {
    if (R <= 0) return;
    const int nb = cull_blocks(R);
    int* count = cull_count_of(ws, R);
    int* totals = count + 1;
    hipLaunchKernelGGL(k_cull_totals, dim3(nb), dim3(CULL_BLOCK), 0, s, lam0, lam1, R, eps, totals);
    hipLaunchKernelGGL(k_cull_emit, dim3(nb), dim3(CULL_BLOCK), 0, s, lam0, lam1, R, eps, totals, cull_map_of(ws, R),
                       cull_slot_of(ws, R), count, count_out);
}

void launch_tp_merge_culled(const float* fg_rgb, const float* fg_depth, const float* lambda, const float* bg_rgb_c,
                            const float* bg_depth_c, const int* slot, int R, float* rgb, float* depth, float* bg_rgb, hipStream_t s) {
    hipLaunchKernelGGL(k_tp_merge_culled, dim3((R + 255) / 256), dim3(256), 0, s, fg_rgb, fg_depth, lambda, bg_rgb_c, bg_depth_c,
                       slot, R, rgb, depth, bg_rgb);
}

}  // namespace neo
