// Decomposed render of NeRF_TP (neo_tp_render_decomposed): the frame of neo_tp_render split into per-instance layers that add up to
// it, an "everything else" layer, and an occlusion-aware id map.  Every level of the frame render is evaluator -> (R,N,4) rgb/sigma
// rows -> k_composite -> resample; the kernel of this file runs AFTER the inside-sphere composite, on what that composite left in
// the lane's scratch - the rows, the sample positions and the scene weights w_j:
//
//   k_tp_decompose       gives every sample of a ray to ONE owner - the lowest-indexed hit instance whose closed interval [lo, hi]
//                        holds it, else the rest - and sums w c, w and w t per owner in k_composite's own order.
//
// The arithmetic is stated in include/neo360_hip.h (DECOMPOSITION RULE).  No evaluator, and not k_composite, is touched: the launch
// list is the dense frame's (tp_render_dense, api_tp.hip) with a full level 0, plus one k_tp_decompose per requested level.
#include "common.h"
#include "tp_frame.h"

using namespace neo_host;

namespace neo {

namespace {

constexpr float DEC_NEAR = 1e-4f;           // neo360/model.py:277
constexpr int DEC_RAYS_PER_BLOCK = 4;       // 4 waves of 64, one ray each (as k_composite)

// the hit rule of objects.hip (obj_lo / obj_hit), per pair
__device__ __forceinline__ float dec_lo(float near) { return near > DEC_NEAR ? near : DEC_NEAR; }

__device__ __forceinline__ bool dec_hit(float n, float f) {
    return !(!(fabsf(n) < __builtin_inff()) || !(fabsf(f) < __builtin_inff()) || !(f > dec_lo(n)));
}

// One wave per ray.  The row is read ONCE, 64 samples a round as in k_composite: lane l keeps the five products of samples l, l + 64,
// ... and their owner in registers (ROUNDS is a template parameter, so the arrays are indexed by unrolled constants only).  Lane
// i < K holds the bounds of pair (i, ray); the slots that are hits on this ray, then the rest (slot K), are summed one after the
// other: per lane in ascending sample order, then wave_sum - k_composite's order, so a slot that owns the whole ray is bitwise its
// rgb / acc / depth (adding 0.0f for a sample of another owner changes nothing).  Lane s keeps slot s's sums and writes them; a
// slot that is no hit on this ray is written as 0.
template <int ROUNDS>
__global__ __launch_bounds__(256) void k_tp_decompose(const float4* __restrict__ rgbsigma, const float* __restrict__ t,
                                                      const float* __restrict__ weights, const float* __restrict__ near_inst,
                                                      const float* __restrict__ far_inst, int K, int R, int N,
                                                      const float* __restrict__ bg_lambda, float* __restrict__ rgb_out,
                                                      float* __restrict__ acc_out, float* __restrict__ depth_out,
                                                      int* __restrict__ id_out) {
    const int ray = blockIdx.x * DEC_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= R) return;
    const int lane = lane_id();
    const float* tr = t + (long)ray * N;
    const float* wr = weights + (long)ray * N;
    const float4* cs = rgbsigma + (long)ray * N;

    float lo = 0.f, hi = 0.f;
    bool hit = false;
    if (lane < K) {
        const float n = near_inst[(long)lane * R + ray], f = far_inst[(long)lane * R + ray];
        hit = dec_hit(n, f);
        lo = dec_lo(n);
        hi = f;
    }
    const unsigned long long hits = __ballot(hit);      // bits 0 .. K-1, K <= 32

    float p_r[ROUNDS], p_g[ROUNDS], p_b[ROUNDS], p_a[ROUNDS], p_d[ROUNDS], tt[ROUNDS];
    int own[ROUNDS];                                    // -1: no sample (beyond N); K: the rest
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int i = r * 64 + lane;
        p_r[r] = p_g[r] = p_b[r] = p_a[r] = p_d[r] = tt[r] = 0.f;
        own[r] = -1;
        if (i < N) {
            const float4 c = cs[i];
            const float w = wr[i], ti = tr[i];
            p_r[r] = w * c.x; p_g[r] = w * c.y; p_b[r] = w * c.z;
            p_a[r] = w;
            p_d[r] = w * ti;
            tt[r] = ti;
            own[r] = K;
        }
    }
    // the owner: the smallest hit i with lo_i <= t_j && t_j <= hi_i (a NaN position is inside nothing)
    for (unsigned long long m = hits; m; m &= m - 1) {
        const int i = __ffsll(m) - 1;
        const float li = __shfl(lo, i, 64), hi_i = __shfl(hi, i, 64);
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r)
            if (own[r] == K && li <= tt[r] && tt[r] <= hi_i) own[r] = i;
    }

    float o_r = 0.f, o_g = 0.f, o_b = 0.f, o_a = 0.f, o_d = 0.f;       // lane s: slot s
    float best = 0.0f, rest_total = 0.0f;
    int id = -1;
    for (unsigned long long m = hits | (1ull << K); m; m &= m - 1) {
        const int s = __ffsll(m) - 1;
        float s_r = 0.f, s_g = 0.f, s_b = 0.f, s_acc = 0.f, s_depth = 0.f;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const bool mine = own[r] == s;
            s_r += mine ? p_r[r] : 0.0f; s_g += mine ? p_g[r] : 0.0f; s_b += mine ? p_b[r] : 0.0f;
            s_acc += mine ? p_a[r] : 0.0f;
            s_depth += mine ? p_d[r] : 0.0f;
        }
        s_r = wave_sum(s_r); s_g = wave_sum(s_g); s_b = wave_sum(s_b);
        s_acc = wave_sum(s_acc); s_depth = wave_sum(s_depth);
        if (lane == s) { o_r = s_r; o_g = s_g; o_b = s_b; o_a = s_acc; o_d = s_depth; }
        if (s < K) {
            if (s_acc > best) { best = s_acc; id = s; }                 // ascending s: ties stay with the lower index; a NaN never wins
        } else {
            rest_total = bg_lambda ? s_acc + bg_lambda[ray] : s_acc;
        }
    }
    if (lane <= K) {
        const long pair = (long)lane * R + ray;
        if (rgb_out) { rgb_out[pair * 3] = o_r; rgb_out[pair * 3 + 1] = o_g; rgb_out[pair * 3 + 2] = o_b; }
        if (acc_out) acc_out[pair] = o_a;
        if (depth_out) depth_out[pair] = o_d;
    }
    if (lane == 0 && id_out) id_out[ray] = (best > 0.0f && best >= rest_total) ? id : -1;
}

}  // namespace

void launch_tp_decompose(const float* rgbsigma, const float* t, const float* weights, const float* near_inst, const float* far_inst,
                         int K, int R, int N, const float* bg_lambda, float* rgb, float* acc, float* depth, int* id, hipStream_t s) {
    if (R <= 0) return;
    const dim3 grid((R + DEC_RAYS_PER_BLOCK - 1) / DEC_RAYS_PER_BLOCK), block(256);
    const int rounds = (N + 63) / 64;
#define NEO_DECOMPOSE(ROUNDS)                                                                                                  \
    hipLaunchKernelGGL(k_tp_decompose<ROUNDS>, grid, block, 0, s, (const float4*)rgbsigma, t, weights, near_inst, far_inst, K, R, \
                       N, bg_lambda, rgb, acc, depth, id)
    if (rounds <= 1) NEO_DECOMPOSE(1);
    else if (rounds <= 2) NEO_DECOMPOSE(2);
    else if (rounds <= 4) NEO_DECOMPOSE(4);
    else if (rounds <= 8) NEO_DECOMPOSE(8);
    else NEO_DECOMPOSE(16);                 // N <= 1024 (checked by the callers)
#undef NEO_DECOMPOSE
}

}  // namespace neo

extern "C" {

// the pure function k_tp_decompose on caller rows; touches no context-owned memory: no ordering scope (as neo_tp_edit_rows)
int neo_tp_decompose_rows(neo_ctx* ctx, const float* rgbsigma, const float* t, const float* weights, const float* near_inst,
                          const float* far_inst, int K, int R, int N, const float* bg_lambda, const neo_tp_decomposed_out* out,
                          void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0 && N >= 1 && N <= 1024, "bad shape (1 <= N <= 1024)");
    REQUIRE(K >= 0 && K <= neo::TP_MAX_EDITS, "0..32 instances supported");
    REQUIRE(static_cast<long>(K + 1) * R * 3 <= 2147483647L, "too many (instance, ray) pairs for 32-bit indices");
    if (R == 0) return NEO_OK;
    REQUIRE(rgbsigma && t && weights, "null pointer");
    REQUIRE(K == 0 || (near_inst && far_inst), "null interval pointer");
    REQUIRE(out, "null output struct");
    neo::launch_tp_decompose(rgbsigma, t, weights, near_inst, far_inst, K, R, N, bg_lambda, out->rgb, out->acc, out->depth, out->id,
                             static_cast<hipStream_t>(stream));
    return check_launch();
}

// the dense frame (tp_render_dense, api_tp.hip) with a full level 0 and k_tp_decompose behind the inside-sphere composite of every
// level that asks for it
int neo_tp_render_decomposed(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, const float* near_inst,
                             const float* far_inst, int K, int R, int chunk, const float* src_poses, int NV, float focal, float cx,
                             float cy, int n_coarse, int n_fine, const neo_tp_level_out* level0, const neo_tp_level_out* level1,
                             const neo_tp_decomposed_out* decomposed0, const neo_tp_decomposed_out* decomposed1,
                             const neo_tp_edit_samples* samples0, const neo_tp_edit_samples* samples1, void* stream) {
    ENTER(ctx);
    REQUIRE(K >= 0 && K <= neo::TP_MAX_EDITS, "0..32 instances supported");
    REQUIRE(static_cast<long>(K + 1) * R * 3 <= 2147483647L, "too many (instance, ray) pairs for 32-bit indices");
    TpDenseOptions o;
    o.level[0] = level0;
    o.level[1] = level1;
    o.near_inst = near_inst;
    o.far_inst = far_inst;
    o.decomposed[0] = decomposed0;
    o.decomposed[1] = decomposed1;
    o.K_dec = K;
    o.samples[0] = samples0;
    o.samples[1] = samples1;
    return tp_render_dense(ctx, {rays_o, rays_d, viewdirs, R, chunk, src_poses, NV, focal, cx, cy, n_coarse, n_fine, stream}, o);
}

}  // extern "C"
