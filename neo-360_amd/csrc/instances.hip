// Instance render of NeRF_TP (neo_tp_render_instances): K per-instance intervals (K, R) - the output of neo_aabb_per_box /
// ops.sample_rays_in_bbox_list - are rendered in ONE call.  Pair (i, ray) is rendered exactly as neo_tp_render_objects renders
// `ray` between near_inst[i], far_inst[i]; the instances of a ray are then composited in depth order, which also gives the
// visible-instance id of the ray.
//
// A compact evaluator launch's row is "ray map[k] with its own sample row", and nothing in the evaluators requires the rays behind
// the rows to be distinct.  So the hit PAIRS (pair = i R + ray, the hit rule of objects.hip per pair) are compacted with the
// two-launch scheme of compact.h over K R elements - stable, no atomics, the count stays on the device - and the pair list is
// consumed in WINDOWS of at most R rows: a compact launch holds at most R rows (its grid is sized from R N, and R is the ray count
// that quirk Q1's last-chunk length reads).  Window p is rows [p R, p R + min(max(count - p R, 0), R)); the host cannot know the
// count, so it enqueues K windows and the empty ones leave at once.  Each window is the launch chain of neo_tp_render_objects on
// the lane's workspaces; its results are scattered straight to their pairs.
//
// This file holds the pair compaction, the level-0 rows of a window, the scatter, the depth-ordered composite and the entry point.
// The evaluators, compositing and resampling in between are the existing kernels on compact rows, untouched.
#include "common.h"
#include "compact.h"
#include "tp_frame.h"

using namespace neo_host;

namespace neo {

namespace {

constexpr int INST_BLOCK = compact::BLOCK;
constexpr float INST_NEAR = 1e-4f;         // neo360/model.py:277

// the hit rule of objects.hip (obj_lo / obj_hit), per pair
__device__ __forceinline__ float inst_lo(float near) { return near > INST_NEAR ? near : INST_NEAR; }

__device__ __forceinline__ bool inst_hit(float n, float f) {
    return !(!(fabsf(n) < __builtin_inff()) || !(fabsf(f) < __builtin_inff()) || !(f > inst_lo(n)));
}

__device__ __forceinline__ bool pair_hit(const float* __restrict__ near_inst, const float* __restrict__ far_inst, int pair, int P) {
    if (pair >= P) return false;
    return inst_hit(near_inst[pair], far_inst[pair]);
}

__global__ __launch_bounds__(INST_BLOCK) void k_inst_totals(const float* __restrict__ near_inst, const float* __restrict__ far_inst,
                                                            int P, int* __restrict__ totals) {
    __shared__ int s_wave[INST_BLOCK / 64];
    compact::totals_body([&](int pair) { return pair_hit(near_inst, far_inst, pair, P); }, s_wave, totals);
}

__global__ __launch_bounds__(INST_BLOCK) void k_inst_emit(const float* __restrict__ near_inst, const float* __restrict__ far_inst,
                                                          int P, const int* __restrict__ totals, int* __restrict__ map,
                                                          int* __restrict__ slot, int* __restrict__ count,
                                                          int* __restrict__ count_out) {
    __shared__ int s_part[INST_BLOCK / 64];
    __shared__ int s_wave[INST_BLOCK / 64];
    compact::emit_body([&](int pair) { return pair_hit(near_inst, far_inst, pair, P); }, P, totals, s_part, s_wave, map, slot, count,
                       count_out);
}

// wcount[p] = rows of window p
__global__ void k_inst_windows(const int* __restrict__ count, int K, int R, int* __restrict__ wcount) {
    const int p = threadIdx.x;
    if (p >= K) return;
    const long left = (long)*count - (long)p * R;
    wcount[p] = left < 0 ? 0 : left > R ? R : (int)left;
}

// k_obj_level0 on a window of the pair list: row k = pair pair_map[k] = (instance, ray); the interval is the pair's, the direction
// the ray's; raymap[k] = ray is what the evaluators read as their map
__global__ void k_inst_level0(const float* __restrict__ near_inst, const float* __restrict__ far_inst,
                              const float* __restrict__ rays_d, const float* __restrict__ edges, const int* __restrict__ pair_map,
                              const int* __restrict__ count, int R, int N, float* __restrict__ t0_c, float* __restrict__ far_c,
                              float* __restrict__ rays_d_c, int* __restrict__ raymap) {
    const long total = (long)*count * N;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int k = (int)(idx / N), i = (int)(idx - (long)k * N);
        const int pair = pair_map[k];
        const float e = edges[i];
        const float near = inst_lo(near_inst[pair]), far = far_inst[pair];
        const float lo = near * (1.0f - e);
        const float hi = far * e;
        t0_c[idx] = lo + hi;
        if (i == 0) {
            const int ray = pair % R;
            raymap[k] = ray;
            far_c[k] = far;
#pragma unroll
            for (int a = 0; a < 3; ++a) rays_d_c[k * 3 + a] = rays_d[ray * 3 + a];
        }
    }
}

__global__ void k_inst_fill_misses(const float* __restrict__ near_inst, const float* __restrict__ far_inst, long P, int white_bkgd,
                                   float* __restrict__ rgb, float* __restrict__ acc, float* __restrict__ depth) {
    for (long pair = (long)blockIdx.x * blockDim.x + threadIdx.x; pair < P; pair += (long)gridDim.x * blockDim.x) {
        if (inst_hit(near_inst[pair], far_inst[pair])) continue;
        const float miss = white_bkgd ? 1.0f : 0.0f;
        if (rgb) {
#pragma unroll
            for (int a = 0; a < 3; ++a) rgb[pair * 3 + a] = miss;
        }
        if (acc) acc[pair] = 0.0f;
        if (depth) depth[pair] = 0.0f;
    }
}

__global__ void k_inst_scatter(const int* __restrict__ pair_map, const int* __restrict__ count, const float* __restrict__ rgb_c,
                               const float* __restrict__ acc_c, const float* __restrict__ depth_c, int white_bkgd,
                               float* __restrict__ prem_rgb, float* __restrict__ prem_acc, float* __restrict__ prem_depth,
                               float* __restrict__ rgb, float* __restrict__ acc, float* __restrict__ depth) {
    const int rows = *count;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < rows; k += gridDim.x * blockDim.x) {
        const long pair = pair_map[k];
        const float a = acc_c[k], d = depth_c[k];
        const float bg = white_bkgd ? 1.0f - a : 0.0f;        // k_composite: rgb += 1 - acc after the sum
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p = rgb_c[k * 3 + c];
            prem_rgb[pair * 3 + c] = p;
            if (rgb) rgb[pair * 3 + c] = white_bkgd ? p + bg : p;
        }
        prem_acc[pair] = a;
        prem_depth[pair] = d;
        if (acc) acc[pair] = a;
        if (depth) depth[pair] = d;
    }
}

// one thread per ray, plain fp32 in the order stated in include/neo360_hip.h (COMPOSITE RECURRENCE)
__global__ void k_inst_composite(const float* __restrict__ near_inst, const float* __restrict__ far_inst, int K, int R,
                                 const float* __restrict__ prem_rgb, const float* __restrict__ prem_acc,
                                 const float* __restrict__ prem_depth, int white_bkgd, float* __restrict__ rgb_out,
                                 float* __restrict__ acc_out, float* __restrict__ depth_out, int* __restrict__ id_out) {
    const int ray = blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= R) return;
    uint32_t left = 0;
    for (int i = 0; i < K; ++i)
        if (inst_hit(near_inst[(long)i * R + ray], far_inst[(long)i * R + ray])) left |= 1u << i;
    float T = 1.0f, r = 0.0f, g = 0.0f, b = 0.0f, depth = 0.0f, acc = 0.0f, best = 0.0f;
    int id = -1;
    while (left) {
        // the nearest remaining instance: ascending lo, ties to the lower index (the scan ascends and replaces on `<` only)
        int i = -1;
        float lo = 0.0f;
        for (int j = 0; j < K; ++j) {
            if (!(left >> j & 1u)) continue;
            const float lj = inst_lo(near_inst[(long)j * R + ray]);
            if (i < 0 || lj < lo) { i = j; lo = lj; }
        }
        left &= ~(1u << i);
        const long pair = (long)i * R + ray;
        const float a = prem_acc[pair];
        const float v = T * a;
        r += T * prem_rgb[pair * 3];
        g += T * prem_rgb[pair * 3 + 1];
        b += T * prem_rgb[pair * 3 + 2];
        depth += T * prem_depth[pair];
        acc += v;
        if (v > best) { best = v; id = i; }
        T = T * (1.0f - a);
    }
    if (white_bkgd) { const float bg = 1.0f - acc; r += bg; g += bg; b += bg; }      // a ray without hits: exactly 1
    if (rgb_out) { rgb_out[ray * 3] = r; rgb_out[ray * 3 + 1] = g; rgb_out[ray * 3 + 2] = b; }
    if (acc_out) acc_out[ray] = acc;
    if (depth_out) depth_out[ray] = depth;
    if (id_out) id_out[ray] = id;
}

inline int grid_for(long total) {
    long blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

}  // namespace

size_t inst_ws_ints(int K, int R) { return cull_ws_ints(K * R) + (size_t)R + (size_t)K; }

void launch_inst_compact(const float* near_inst, const float* far_inst, int K, int R, int* ws, int* count_out, hipStream_t s) {
    const int P = K * R;
    if (P <= 0) return;
    const int nb = compact::blocks(P);
    int* count = cull_count_of(ws, P);
    int* totals = count + 1;
    hipLaunchKernelGGL(k_inst_totals, dim3(nb), dim3(INST_BLOCK), 0, s, near_inst, far_inst, P, totals);
    hipLaunchKernelGGL(k_inst_emit, dim3(nb), dim3(INST_BLOCK), 0, s, near_inst, far_inst, P, totals, cull_map_of(ws, P),
                       cull_slot_of(ws, P), count, count_out);
    hipLaunchKernelGGL(k_inst_windows, dim3(1), dim3(64), 0, s, count, K, R, inst_wcount_of(ws, K, R));
}

void launch_inst_level0(const float* near_inst, const float* far_inst, const float* rays_d, const float* edges, const int* pair_map,
                        const int* count, int R, int N, float* t0_c, float* far_c, float* rays_d_c, int* raymap, hipStream_t s) {
    if (R <= 0) return;
    hipLaunchKernelGGL(k_inst_level0, dim3(grid_for((long)R * N)), dim3(256), 0, s, near_inst, far_inst, rays_d, edges, pair_map, count,
                       R, N, t0_c, far_c, rays_d_c, raymap);
}

void launch_inst_fill_misses(const float* near_inst, const float* far_inst, long pairs, int white_bkgd, float* rgb, float* acc,
                             float* depth, hipStream_t s) {
    if (pairs <= 0 || !(rgb || acc || depth)) return;
    hipLaunchKernelGGL(k_inst_fill_misses, dim3(grid_for(pairs)), dim3(256), 0, s, near_inst, far_inst, pairs, white_bkgd, rgb, acc,
                       depth);
}

void launch_inst_scatter(const int* pair_map, const int* count, int R, const float* rgb_c, const float* acc_c, const float* depth_c,
                         int white_bkgd, float* prem_rgb, float* prem_acc, float* prem_depth, float* rgb, float* acc, float* depth,
                         hipStream_t s) {
    if (R <= 0) return;
    hipLaunchKernelGGL(k_inst_scatter, dim3(grid_for(R)), dim3(256), 0, s, pair_map, count, rgb_c, acc_c, depth_c, white_bkgd, prem_rgb,
                       prem_acc, prem_depth, rgb, acc, depth);
}

void launch_inst_composite(const float* near_inst, const float* far_inst, int K, int R, const float* prem_rgb, const float* prem_acc,
                           const float* prem_depth, int white_bkgd, float* rgb, float* acc, float* depth, int* instance_id,
                           hipStream_t s) {
    if (R <= 0 || !(rgb || acc || depth || instance_id)) return;
    hipLaunchKernelGGL(k_inst_composite, dim3((R + 255) / 256), dim3(256), 0, s, near_inst, far_inst, K, R, prem_rgb, prem_acc,
                       prem_depth, white_bkgd, rgb, acc, depth, instance_id);
}

}  // namespace neo

extern "C" {

// Every instance of a scene in one call: hit rule, windows and the composite recurrence are stated in include/neo360_hip.h.
int neo_tp_render_instances(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, const float* near_inst,
                            const float* far_inst, int K, int R, int chunk, const float* src_poses, int NV, float focal, float cx,
                            float cy, int n_coarse, int n_fine, int white_bkgd, const neo_tp_instance_out* level0,
                            const neo_tp_instance_out* level1, int* pairs_out, void* stream) {
    ENTER(ctx);
    const TpFrameArgs a{rays_o, rays_d, viewdirs, R, chunk, src_poses, NV, focal, cx, cy, n_coarse, n_fine, stream};
    TpFrame::Own own;
    if (!(K >= 0 && K <= 32)) own.after_rays = "0..32 instances supported";
    else if (!(static_cast<long>(K) * R * 3 <= 2147483647L)) own.after_rays = "too many (instance, ray) pairs for 32-bit indices";
    own.empty = K == 0;
    own.ptrs = near_inst && far_inst;
    TpFrame f;      // no outside-sphere slots, no ray-grid hint: every launch is compact
    if (int rc = f.begin(ctx, a, false, false, own)) return rc;
    hipStream_t s = f.s;
    if (f.empty) {
        if (pairs_out) HIP_TRY(hipMemsetAsync(pairs_out, 0, sizeof(int), s));
        if (R == 0) return NEO_OK;
        // no instances: the composite of a ray without hits (the kernel reads no input when K == 0)
        for (const neo_tp_instance_out* lv : {level0, level1})
            if (lv)
                neo::launch_inst_composite(nullptr, nullptr, 0, R, nullptr, nullptr, nullptr, white_bkgd ? 1 : 0, lv->comp_rgb,
                                           lv->comp_acc, lv->comp_depth, lv->instance_id, s);
        return check_launch();
    }

    // workspaces: this lane's set.  `c` is one WINDOW's compact rows, as in neo_tp_render_objects (sized for R rows and reused by
    // every window: the stream orders them); W[4] keeps every pair's un-whitened results of both levels for the composite, W[10]
    // the pair compaction, the current window's ray map and the window counts.
    auto* W = ctx->ws;
    const size_t r = static_cast<size_t>(R), pairs = static_cast<size_t>(K) * r;
    TpCompactRows c;
    if (c.reserve(W, r, f.N0, f.N1) || W[4].reserve(pairs * 10 * 4) || W[10].reserve(neo::inst_ws_ints(K, R) * sizeof(int)))
        return NEO_ERR_NOMEM;
    float* prem = W[4].as<float>();       // per level: rgb(3) acc depth = 5 floats a pair
    int* cws = W[10].as<int>();
    const int P = K * R;
    const int* pair_map = neo::cull_map_of(cws, P);
    int* raymap = neo::inst_raymap_of(cws, K, R);
    const int* wcount = neo::inst_wcount_of(cws, K, R);
    float* p_rgb[2] = {prem, prem + pairs * 5};
    float* p_acc[2] = {prem + pairs * 3, prem + pairs * 8};
    float* p_depth[2] = {prem + pairs * 4, prem + pairs * 9};
    const neo_tp_instance_out* lv[2] = {level0, level1};
    const int white = white_bkgd ? 1 : 0;

    neo::launch_inst_compact(near_inst, far_inst, K, R, cws, pairs_out, s);
    for (int l = 0; l < 2; ++l)
        if (lv[l]) neo::launch_inst_fill_misses(near_inst, far_inst, static_cast<long>(P), white, lv[l]->rgb, lv[l]->acc, lv[l]->depth, s);
    for (int p = 0; p < K; ++p) {
        // grids sized for R, every kernel takes its row count from the window's device word
        const int* map_w = pair_map + static_cast<size_t>(p) * r;
        const int* count = wcount + p;
        neo::launch_inst_level0(near_inst, far_inst, rays_d, f.edges, map_w, count, R, f.N0, c.t0, c.far, c.rays_d, raymap, s);
        // composited WITHOUT white: the scatter adds 1 - acc to the per-instance rows, the composite below needs them without it
        if (int rc = tp_march_compact(f, a, c, raymap, count, 0)) return rc;
        for (int l = 0; l < 2; ++l)
            neo::launch_inst_scatter(map_w, count, R, c.rgb[l], c.acc[l], c.depth[l], white, p_rgb[l], p_acc[l], p_depth[l],
                                     lv[l] ? lv[l]->rgb : nullptr, lv[l] ? lv[l]->acc : nullptr, lv[l] ? lv[l]->depth : nullptr, s);
    }
    for (int l = 0; l < 2; ++l)
        if (lv[l])
            neo::launch_inst_composite(near_inst, far_inst, K, R, p_rgb[l], p_acc[l], p_depth[l], white, lv[l]->comp_rgb,
                                       lv[l]->comp_acc, lv[l]->comp_depth, lv[l]->instance_id, s);
    return check_launch();
}

}  // extern "C"
