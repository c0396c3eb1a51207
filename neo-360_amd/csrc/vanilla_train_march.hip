// Training through the vanilla occupancy grid (include/neo360_hip.h: VANILLA MARCHING TRAINING).  The training chain
// neo_vanilla_mlp_train_forward / _backward works on arbitrary rows, each with its own cond; what this file adds around it:
//
//   k_vt_rows               the compact row builder: behind the keep mask and totals of the (R,N) samples of one level (the BOX
//                           KEEP RULE, launch_point_keep of point_list.hip), for the kept ones - in ascending flat order, by
//                           occ_rank - their flat index, their 63-d position encoding (k_pos_enc's per-feature expression) and
//                           their ray's direction encoding;
//   k_vt_scatter / _bwd     the output activations (neo_tp_activate's expressions) fused with the scatter into the composite's
//                           zero-filled (R N, 4) rows, and the gather + activation backward;
//   k_vt_probes             one jittered probe point per cell of the BOX GRID, from the library's counter-based generator;
//   k_vt_density            the running density of the grid: max(decay density, max(sigma0, sigma1)), NaN-propagating.
//
// A workgroup of the row builder owns OCC_POINTS consecutive samples; its kept samples are consecutive compact rows, so the 63 + 27
// floats of each are written as ONE contiguous run per workgroup (point coordinates staged in LDS, one feature per thread and
// store), not as 252-byte strided rows per thread.  No atomics, no spinning; the results do not depend on the launch geometry.
#include "common.h"
#include "ctx.h"
#include "march.h"
#include "occ_points.h"
#include "philox.h"

using namespace neo_host;

namespace neo {

namespace {

constexpr int VT_PE = 63, VT_COND = 27;      // pos_enc(x, 0, 10) of a 3-d point, pos_enc(d, 0, 4) of a direction
constexpr uint32_t VT_PROBE_STREAM = 8;      // streams 0..7 are the samplers' (training.py: _draws); 8, 9, 10 = the probe's x, y, z

__global__ __launch_bounds__(OCC_BLOCK) void k_vt_rows(const float* __restrict__ rays_o, const float* __restrict__ dirs,
                                                       const float* __restrict__ t, const float* __restrict__ dir_enc,
                                                       const uint8_t* __restrict__ keep, int N, int P,
                                                       const int* __restrict__ totals, int cap, int* __restrict__ count,
                                                       int* __restrict__ index, float* __restrict__ x_enc,
                                                       float* __restrict__ cond) {
    __shared__ int s_part[OCC_BLOCK / 64];
    __shared__ int s_seg[OCC_SEGS];
    __shared__ float s_x[OCC_POINTS * 3];      // the kept points of this workgroup, by local rank
    __shared__ int s_ray[OCC_POINTS];
    const OccRank rk = occ_rank(keep, P, totals, s_part, s_seg);
    const int first = rk.upto - totals[blockIdx.x];      // compact row of this workgroup's first kept sample
#pragma unroll
    for (int it = 0; it < OCC_ROUNDS; ++it) {
        if (!rk.kept[it]) continue;
        const int p = blockIdx.x * OCC_POINTS + it * OCC_BLOCK + threadIdx.x;
        const int ray = p / N, l = rk.k[it] - first;
        const float tv = t[p];
#pragma unroll
        for (int a = 0; a < 3; ++a) s_x[l * 3 + a] = rays_o[(long)ray * 3 + a] + tv * dirs[(long)ray * 3 + a];      // mul then add
        s_ray[l] = ray;
        if (rk.k[it] < cap) index[rk.k[it]] = p;
    }
    __syncthreads();
    const int live = min(rk.upto, cap) - first;      // rows of this workgroup in front of the cap (may be <= 0)
    for (int i = threadIdx.x; i < live * VT_PE; i += OCC_BLOCK) {
        const int l = i / VT_PE, f = i - l * VT_PE;
        x_enc[(long)first * VT_PE + i] = pos_enc_feature([&](int c) { return s_x[l * 3 + c]; }, 3, 0, 10, f);
    }
    for (int i = threadIdx.x; i < live * VT_COND; i += OCC_BLOCK) {
        const int l = i / VT_COND, f = i - l * VT_COND;
        cond[(long)first * VT_COND + i] = dir_enc[(long)s_ray[l] * VT_COND + f];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *count = rk.upto;
}

// packed[index[k]] = neo_tp_activate's row of (raw_rgb[k], raw_sigma[k], noise[index[k]]); an index outside [0, P) writes nothing
__global__ void k_vt_scatter(const float* __restrict__ raw_rgb, const float* __restrict__ raw_sigma, const int* __restrict__ index,
                             long K, const float* __restrict__ noise, float noise_scale, long P, float4* __restrict__ packed) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const long p = index[k];
    if (p < 0 || p >= P) return;
    const float rs = raw_sigma[k] + (noise ? noise[p] * noise_scale : 0.0f);
    packed[p] = make_float4(colour_act(raw_rgb[k * 3]), colour_act(raw_rgb[k * 3 + 1]), colour_act(raw_rgb[k * 3 + 2]), density_act(rs));
}

// neo_tp_activate_backward on the gathered rows g[index[k]]; an index outside [0, P) gives zero gradients
__global__ void k_vt_scatter_bwd(const float* __restrict__ raw_rgb, const float* __restrict__ raw_sigma, const int* __restrict__ index,
                                 long K, const float* __restrict__ noise, float noise_scale, long P, const float4* __restrict__ g,
                                 float* __restrict__ g_rgb, float* __restrict__ g_sigma) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const long p = index[k];
    const bool in = p >= 0 && p < P;
    const float4 gi = in ? g[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float gc[3] = {gi.x, gi.y, gi.z};
#pragma unroll
    for (int c = 0; c < 3; ++c) g_rgb[k * 3 + c] = colour_act_grad(raw_rgb[k * 3 + c], gc[c]);
    const float x = raw_sigma[k] + (noise && in ? noise[p] * noise_scale : 0.0f) + (-1.0f);
    g_sigma[k] = density_act_grad(x, gi.w);
}

// PROBE POINTS: per axis lo + (c + u) w with w = (hi - lo) / G formed once on the host; a candidate whose own fp32 cell
// floorf((x - lo) scale) is not c is replaced by the centre lo + (c + 0.5) w of that axis
struct VtProbeBox {
    float lo[3], w[3], scale[3];
};
__global__ void k_vt_probes(VtProbeBox b, int G, uint64_t seed, uint32_t step, float* __restrict__ pts) {
    const int cells = G * G * G;
    const int lin = blockIdx.x * blockDim.x + threadIdx.x;
    if (lin >= cells) return;
    const int c[3] = {lin / (G * G), (lin / G) % G, lin % G};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float u = philox_uniform(seed, (uint32_t)lin, step, VT_PROBE_STREAM + a);
        float x = b.lo[a] + ((float)c[a] + u) * b.w[a];
        if (floorf((x - b.lo[a]) * b.scale[a]) != (float)c[a]) x = b.lo[a] + ((float)c[a] + 0.5f) * b.w[a];
        pts[(long)lin * 3 + a] = x;
    }
}

// the larger of two densities, a NaN on either side winning (torch.maximum)
__device__ __forceinline__ float vt_nanmax(float a, float b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }

__global__ void k_vt_density(float* __restrict__ density, const float* __restrict__ sigma0, const float* __restrict__ sigma1,
                             float decay, int cells) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells) return;
    const float s = sigma1 ? vt_nanmax(sigma0[i], sigma1[i]) : sigma0[i];
    density[i] = vt_nanmax(decay * density[i], s);
}

}  // namespace

}  // namespace neo

extern "C" {

// writes one lane workspace (the per-workgroup totals of the compaction): ordered like every lane call
int neo_vanilla_train_rows(neo_ctx* ctx, const uint32_t* bits, int G, const float* lo, const float* hi, int clip, const float* rays_o,
                           const float* dirs, const float* t, const float* dir_enc, int R, int N, int cap, uint8_t* keep, int* count,
                           int* index, float* x_enc, float* cond, void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0 && N >= 1 && cap >= 0, "bad shape");
    REQUIRE(static_cast<long>(R) * N <= 2147483647L - 1024, "too many points for 32-bit indices");
    REQUIRE(count, "null pointer");
    neo::OccGrid box{};
    if (bits) {
        REQUIRE(neo::occ_resolution_ok(G), neo::OCC_RESOLUTION_MSG);
        REQUIRE(lo && hi, "null pointer");
        if (const char* msg = neo::occ_grid_box(G, lo, hi, clip, box)) return fail(NEO_ERR_INVALID, "%s", msg);
        box.bits = bits;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (R == 0) {
        HIP_TRY(hipMemsetAsync(count, 0, sizeof(int), s));
        return NEO_OK;
    }
    REQUIRE(rays_o && dirs && t && dir_enc && keep, "null pointer");
    REQUIRE(cap == 0 || (index && x_enc && cond), "null pointer");
    const int P = R * N;
    const int nb = neo::occ_blocks(P);
    ORDERED_LANE(ctx, s);
    if (ctx->ws[5].reserve(static_cast<size_t>(nb) * sizeof(int))) return NEO_ERR_NOMEM;
    int* totals = ctx->ws[5].as<int>();
    neo::launch_point_keep(neo::point_source_dense(rays_o, dirs, t, N, R, N), box, keep, totals, s);
    hipLaunchKernelGGL(neo::k_vt_rows, dim3(nb), dim3(neo::OCC_BLOCK), 0, s, rays_o, dirs, t, dir_enc, (const uint8_t*)keep, N, P,
                       (const int*)totals, cap, count, index, x_enc, cond);
    return check_launch();
}

int neo_vanilla_train_scatter(neo_ctx* ctx, const float* raw_rgb, const float* raw_sigma, const int* index, long K, const float* noise,
                              float noise_scale, long P, float* packed, void* stream) {
    ENTER(ctx);
    REQUIRE(K >= 0 && P >= 0 && K <= P, "bad shape (0 <= K <= P)");
    REQUIRE(P <= 2147483647L, "too many points for 32-bit indices");
    if (P == 0) return NEO_OK;
    REQUIRE(packed, "null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(packed, 0, static_cast<size_t>(P) * 16, s));
    if (K == 0) return NEO_OK;
    REQUIRE(raw_rgb && raw_sigma && index, "null pointer");
    hipLaunchKernelGGL(neo::k_vt_scatter, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, raw_rgb, raw_sigma, index, K, noise,
                       noise_scale, P, reinterpret_cast<float4*>(packed));
    return check_launch();
}

int neo_vanilla_train_scatter_backward(neo_ctx* ctx, const float* raw_rgb, const float* raw_sigma, const int* index, long K,
                                       const float* noise, float noise_scale, long P, const float* g_packed, float* g_rgb,
                                       float* g_sigma, void* stream) {
    ENTER(ctx);
    REQUIRE(K >= 0 && P >= 0 && K <= P, "bad shape (0 <= K <= P)");
    REQUIRE(P <= 2147483647L, "too many points for 32-bit indices");
    if (K == 0) return NEO_OK;
    REQUIRE(raw_rgb && raw_sigma && index && g_packed && g_rgb && g_sigma, "null pointer");
    hipLaunchKernelGGL(neo::k_vt_scatter_bwd, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), raw_rgb,
                       raw_sigma, index, K, noise, noise_scale, P, reinterpret_cast<const float4*>(g_packed), g_rgb, g_sigma);
    return check_launch();
}

int neo_vanilla_grid_probes(neo_ctx* ctx, int G, const float* lo, const float* hi, uint64_t seed, uint32_t step, float* pts,
                            void* stream) {
    ENTER(ctx);
    REQUIRE(neo::occ_resolution_ok(G), neo::OCC_RESOLUTION_MSG);
    REQUIRE(lo && hi && pts, "null pointer");
    neo::OccGrid box{};
    if (const char* msg = neo::occ_grid_box(G, lo, hi, 0, box)) return fail(NEO_ERR_INVALID, "%s", msg);
    neo::VtProbeBox pb{};
    for (int a = 0; a < 3; ++a) {
        pb.lo[a] = box.lo[a];
        pb.scale[a] = box.scale[a];
        pb.w[a] = (hi[a] - lo[a]) / static_cast<float>(G);
        // a cell must hold its own centre in fp32: the centre and the cell expression each miss the real value by a few ulp of
        // the box's largest coordinate, so 64 of them per cell leave the centre more than a quarter of a cell from either face
        const float big = std::fmax(std::fabs(lo[a]), std::fabs(hi[a]));
        REQUIRE(pb.w[a] > 0.0f && pb.w[a] < INFINITY && pb.w[a] * 131072.0f >= big,
                "the box's cells are too thin for fp32 probe points (a cell needs 64 ulp of the box's largest coordinate)");
    }
    const int cells = G * G * G;
    hipLaunchKernelGGL(neo::k_vt_probes, dim3((cells + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), pb, G, seed, step, pts);
    return check_launch();
}

int neo_vanilla_density_update(neo_ctx* ctx, float* density, const float* sigma0, const float* sigma1, int G, float decay, void* stream) {
    ENTER(ctx);
    REQUIRE(neo::occ_resolution_ok(G), neo::OCC_RESOLUTION_MSG);
    REQUIRE(decay >= 0.0f && decay <= 1.0f, "decay must lie in [0, 1]");
    REQUIRE(density && sigma0, "null pointer");
    const int cells = G * G * G;
    hipLaunchKernelGGL(neo::k_vt_density, dim3((cells + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), density, sigma0,
                       sigma1, decay, cells);
    return check_launch();
}

}  // extern "C"
