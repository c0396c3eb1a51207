// Edited render of NeRF_TP (neo_tp_render_edited): the scene WITHOUT an instance, or with an instance faded, recoloured or standing
// somewhere else.  Every level of the frame render is evaluator -> (R,N,4) rgb/sigma rows -> k_composite -> resample; the two
// kernels of this file sit between the inside-sphere evaluator and its composite:
//
//   k_tp_edit            multiplies sigma and rgb of the samples that lie inside a per-instance interval [lo, hi] of their ray by
//                        that instance's density scale and tint (scale 0 removes it), in place;
//   k_composite_layers   mode 1 of k_composite (sampling.hip) with up to 32 per-ray LAYERS - an opacity, a premultiplied colour and
//                        a premultiplied depth at a ray parameter `key`, e.g. an instance rendered somewhere else by
//                        neo_tp_render_objects - spliced into the ray in depth order.
//
// The arithmetic of both is stated in include/neo360_hip.h (EDIT RULE, LAYER RECURRENCE).  No evaluator, and not k_composite, is
// touched: without edits and layers the launch list (tp_render_dense, api_tp.hip) is neo_tp_render's with a full level 0.
#include "common.h"
#include "tp_frame.h"

using namespace neo_host;

namespace neo {

namespace {

constexpr float EDIT_NEAR = 1e-4f;          // neo360/model.py:277
constexpr int LAYER_RAYS_PER_BLOCK = 4;     // 4 waves of 64, one ray each (as k_composite)

// the hit rule of objects.hip (obj_lo / obj_hit), per pair
__device__ __forceinline__ float edit_lo(float near) { return near > EDIT_NEAR ? near : EDIT_NEAR; }

__device__ __forceinline__ bool edit_hit(float n, float f) {
    return !(!(fabsf(n) < __builtin_inff()) || !(fabsf(f) < __builtin_inff()) || !(f > edit_lo(n)));
}

// One thread per sample, one coalesced float4 pass; the K bounds of a ray are the same words for all its samples (cache hits).
// A sample inside no interval is not written.
__global__ __launch_bounds__(256) void k_tp_edit(float4* __restrict__ rgbsigma, const float* __restrict__ t,
                                                 const float* __restrict__ near_inst, const float* __restrict__ far_inst, int K,
                                                 long R, int N, TpEditTable tab) {
    const long total = R * N;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long ray = idx / N;
        const float tj = t[idx];
        float4 c = rgbsigma[idx];
        bool touched = false;
        for (int i = 0; i < K; ++i) {
            const float n = near_inst[(long)i * R + ray], f = far_inst[(long)i * R + ray];
            if (!edit_hit(n, f)) continue;
            if (edit_lo(n) <= tj && tj <= f) {          // the closed interval: render_objects places samples on both ends
                c.w *= tab.scale[i];
                c.x *= tab.tint[i][0];
                c.y *= tab.tint[i][1];
                c.z *= tab.tint[i][2];
                touched = true;
            }
        }
        if (touched) rgbsigma[idx] = c;
    }
}

// k_composite mode 1 with L <= 32 layers of the ray: one wave per ray, 64-sample rounds, fp64 transmittance carry.
// Lane p < nvalid owns the p-th valid layer in (key, index) order; lane p <= nvalid holds pfx = the fp64 product of the first p
// keeps, multiplied left to right.  The per-sample lines are k_composite's, so that a ray without a valid layer is bitwise its
// result ((carry * excl) * 1.0 is exact).
__global__ __launch_bounds__(256) void k_composite_layers(const float4* __restrict__ rgbsigma, const float* __restrict__ t,
                                                          const float* __restrict__ rays_d, const float* __restrict__ t_far, int R,
                                                          int N, const float* __restrict__ l_key, const float* __restrict__ l_rgb,
                                                          const float* __restrict__ l_acc, const float* __restrict__ l_depth, int L,
                                                          float* __restrict__ rgb_out, float* __restrict__ acc_out,
                                                          float* __restrict__ depth_out, float* __restrict__ w_out,
                                                          float* __restrict__ lambda_out, float* __restrict__ vis_out) {
    const int ray = blockIdx.x * LAYER_RAYS_PER_BLOCK + (threadIdx.x >> 6);
    if (ray >= R) return;
    const int lane = lane_id();
    const float* tr = t + (long)ray * N;
    const float4* cs = rgbsigma + (long)ray * N;
    const float dx = rays_d[ray * 3], dy = rays_d[ray * 3 + 1], dz = rays_d[ray * 3 + 2];
    const float dnorm = sqrtf(dx * dx + dy * dy + dz * dz);
    const float far = t_far[ray];

    // ---- the ray's layers: validity, order, prefix products ----
    float key = 0.f, la = 0.f;
    bool lvalid = false;
    if (lane < L) {
        key = l_key[(long)lane * R + ray];
        la = l_acc[(long)lane * R + ray];
        lvalid = !(!(fabsf(key) < __builtin_inff()) || !(la > 0.0f));      // a NaN key or opacity is invalid
    }
    const int nvalid = __popcll(__ballot(lvalid));
    int rank = 0;                       // valid layers ordered before this one: ascending key, ties to the lower index
    for (int m = 0; m < L; ++m) {
        const float km = __shfl(key, m, 64);
        const int vm = __shfl((int)lvalid, m, 64);
        if (vm && (km < key || (km == key && m < lane))) rank += 1;
    }
    int src = 0;                        // lane p < nvalid: the index of the layer at position p
    for (int m = 0; m < L; ++m) {
        const int rm = __shfl(rank, m, 64);
        const int vm = __shfl((int)lvalid, m, 64);
        if (vm && rm == lane) src = m;
    }
    const bool owner = lane < nvalid;
    const float skey = __shfl(key, src, 64);
    const float sa = __shfl(la, src, 64);
    float keepf = 1.0f - sa;
    keepf = keepf > 0.0f ? keepf : 0.0f;
    const double skeep = owner ? (double)keepf : 1.0;
    double pfx = 1.0;
    for (int q = 0; q < nvalid; ++q) {
        const double kq = __shfl(skeep, q, 64);
        if (q < lane) pfx = pfx * kq;
    }
    double s_at = 1.0;                  // owner: the scene's transmittance before the first sample at or beyond its key
    uint32_t placed = 0;                // uniform: layers whose sample has been found

    double carry = 1.0;  // product of (1-alpha+eps) over all earlier samples
    float s_r = 0.f, s_g = 0.f, s_b = 0.f, s_acc = 0.f, s_depth = 0.f;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        const bool valid = i < N;
        float alpha = 0.f, ti = 0.f;
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid) {
            ti = tr[i];
            c = cs[i];
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
        double excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0;
        const double scene = carry * excl;                  // S(j)
        // layers at or before this sample are a prefix of the order; each layer meets its first sample at or beyond its key
        int before = 0;
        for (int q = 0; q < nvalid; ++q) {
            const float kq = __shfl(skey, q, 64);
            const bool at = valid && ti >= kq;
            before += at ? 1 : 0;
            if (!(placed >> q & 1u)) {
                const unsigned long long m = __ballot(at);
                if (m) {
                    const int first = __ffsll(m) - 1;
                    const double sv = __shfl(scene, first, 64);
                    if (lane == q) s_at = sv;
                    placed |= 1u << q;
                }
            }
        }
        const double front = __shfl(pfx, before, 64);       // A(j)
        // per-element rounding to fp32 mirrors storing the fp32 cumprod tensor
        const float trans_scene = (float)scene;
        const float trans = (float)(scene * front);
        const float w = alpha * trans;
        carry = carry * __shfl(incl, 63, 64);
        if (valid) {
            if (w_out) w_out[(long)ray * N + i] = alpha * trans_scene;
            s_r += w * c.x; s_g += w * c.y; s_b += w * c.z;
            s_acc += w;
            s_depth += w * ti;
        }
    }
    if (owner) {
        if (!(placed >> lane & 1u)) s_at = carry;           // beyond the last sample: behind the whole scene
        const float v = (float)(s_at * pfx);
        const long pair = (long)src * R + ray;
        s_r += v * l_rgb[pair * 3]; s_g += v * l_rgb[pair * 3 + 1]; s_b += v * l_rgb[pair * 3 + 2];
        s_acc += v * sa;
        s_depth += v * l_depth[pair];
        if (vis_out) vis_out[pair] = v * sa;
    }
    if (vis_out && lane < L && !lvalid) vis_out[(long)lane * R + ray] = 0.0f;
    const double all_keeps = __shfl(pfx, nvalid, 64);
    s_r = wave_sum(s_r); s_g = wave_sum(s_g); s_b = wave_sum(s_b);
    s_acc = wave_sum(s_acc); s_depth = wave_sum(s_depth);
    if (lane == 0) {
        if (rgb_out) { rgb_out[ray * 3] = s_r; rgb_out[ray * 3 + 1] = s_g; rgb_out[ray * 3 + 2] = s_b; }
        if (acc_out) acc_out[ray] = s_acc;
        if (depth_out) depth_out[ray] = s_depth;
        if (lambda_out) lambda_out[ray] = (float)(carry * all_keeps);
    }
}

}  // namespace

void launch_tp_edit(float* rgbsigma, const float* t, const float* near_inst, const float* far_inst, int K, int R, int N,
                    const TpEditTable& tab, hipStream_t s) {
    if (K <= 0 || R <= 0 || N <= 0) return;
    long blocks = ((long)R * N + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(k_tp_edit, dim3((int)blocks), dim3(256), 0, s, (float4*)rgbsigma, t, near_inst, far_inst, K, (long)R, N, tab);
}

void launch_composite_layers(const float* rgbsigma, const float* t, const float* rays_d, const float* t_far, int R, int N,
                             const float* l_key, const float* l_rgb, const float* l_acc, const float* l_depth, int L, float* rgb,
                             float* acc, float* depth, float* weights, float* lambda, float* visibility, hipStream_t s) {
    if (R <= 0) return;
    hipLaunchKernelGGL(k_composite_layers, dim3((R + LAYER_RAYS_PER_BLOCK - 1) / LAYER_RAYS_PER_BLOCK), dim3(256), 0, s,
                       (const float4*)rgbsigma, t, rays_d, t_far, R, N, l_key, l_rgb, l_acc, l_depth, L, rgb, acc, depth, weights,
                       lambda, visibility);
}

}  // namespace neo

namespace {

// the host table of an edit: K scales and K x 3 tints, finite and >= 0 (NULL = all ones)
int fill_edit_table(neo::TpEditTable& tab, int K, const float* density_scale, const float* tint) {
    for (int i = 0; i < neo::TP_MAX_EDITS; ++i) {
        tab.scale[i] = 1.0f;
        for (int c = 0; c < 3; ++c) tab.tint[i][c] = 1.0f;
    }
    for (int i = 0; i < K; ++i) {
        if (density_scale) {
            REQUIRE(std::isfinite(density_scale[i]) && density_scale[i] >= 0.0f, "density scales must be finite and >= 0");
            tab.scale[i] = density_scale[i];
        }
        if (tint)
            for (int c = 0; c < 3; ++c) {
                REQUIRE(std::isfinite(tint[i * 3 + c]) && tint[i * 3 + c] >= 0.0f, "tints must be finite and >= 0");
                tab.tint[i][c] = tint[i * 3 + c];
            }
    }
    return NEO_OK;
}

}  // namespace

extern "C" {

// the pure function k_tp_edit on caller rows; touches no context-owned memory: no ordering scope (as neo_tp_extras)
int neo_tp_edit_rows(neo_ctx* ctx, float* rgbsigma, const float* t, const float* near_inst, const float* far_inst, int K,
                     const float* density_scale, const float* tint, int R, int N, void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0 && N >= 1, "bad shape");
    REQUIRE(K >= 0 && K <= neo::TP_MAX_EDITS, "0..32 instances supported");
    REQUIRE(static_cast<long>(K) * R <= 2147483647L, "too many (instance, ray) pairs for 32-bit indices");
    neo::TpEditTable tab;
    if (int rc = fill_edit_table(tab, K, density_scale, tint)) return rc;
    if (R == 0 || K == 0) return NEO_OK;
    REQUIRE(rgbsigma && t && near_inst && far_inst, "null pointer");
    neo::launch_tp_edit(rgbsigma, t, near_inst, far_inst, K, R, N, tab, static_cast<hipStream_t>(stream));
    return check_launch();
}

// the pure function k_composite_layers on caller rows; touches no context-owned memory: no ordering scope (as neo_composite)
int neo_composite_layers(neo_ctx* ctx, const float* rgbsigma, const float* t, const float* rays_d, const float* t_far, int R, int N,
                         const neo_tp_layers* layers, int L, float* rgb, float* acc, float* depth, float* weights, float* lambda,
                         float* visibility, void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0 && N >= 1, "bad shape");
    REQUIRE(L >= 0 && L <= neo::TP_MAX_EDITS, "0..32 layers supported");
    REQUIRE(static_cast<long>(L) * R * 3 <= 2147483647L, "too many (layer, ray) pairs for 32-bit indices");
    if (R == 0) return NEO_OK;
    REQUIRE(rgbsigma && t && rays_d && t_far, "null pointer");
    REQUIRE(L == 0 || (layers && layers->key && layers->rgb && layers->acc && layers->depth), "null layer pointer");
    neo::launch_composite_layers(rgbsigma, t, rays_d, t_far, R, N, L ? layers->key : nullptr, L ? layers->rgb : nullptr,
                                 L ? layers->acc : nullptr, L ? layers->depth : nullptr, L, rgb, acc, depth, weights, lambda,
                                 visibility, static_cast<hipStream_t>(stream));
    return check_launch();
}

// the dense frame (tp_render_dense, api_tp.hip) with a full level 0, k_tp_edit on the inside-sphere rows of each level before their
// composite and k_composite_layers as that composite when layers are given
int neo_tp_render_edited(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, const float* near_inst,
                         const float* far_inst, int K, const float* density_scale, const float* tint, const neo_tp_layers* layers,
                         int L, int R, int chunk, const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse,
                         int n_fine, const neo_tp_level_out* level0, const neo_tp_level_out* level1,
                         const neo_tp_edit_samples* samples0, const neo_tp_edit_samples* samples1, void* stream) {
    ENTER(ctx);
    REQUIRE(K >= 0 && K <= neo::TP_MAX_EDITS, "0..32 instances supported");
    REQUIRE(L >= 0 && L <= neo::TP_MAX_EDITS, "0..32 layers supported");
    REQUIRE(static_cast<long>(K > L ? K : L) * R * 3 <= 2147483647L, "too many (instance, ray) pairs for 32-bit indices");
    neo::TpEditTable tab;
    if (int rc = fill_edit_table(tab, K, density_scale, tint)) return rc;
    TpDenseOptions o;
    o.level[0] = level0;
    o.level[1] = level1;
    o.near_inst = near_inst;
    o.far_inst = far_inst;
    o.edit = &tab;
    o.K_edit = K;
    o.layers = layers;
    o.L = L;
    o.samples[0] = samples0;
    o.samples[1] = samples1;
    return tp_render_dense(ctx, {rays_o, rays_d, viewdirs, R, chunk, src_poses, NV, focal, cx, cy, n_coarse, n_fine, stream}, o);
}

}  // extern "C"
