// Empty-space skipping and early ray termination of the VANILLA frame (neo_vanilla_render_marching; include/neo360_hip.h: VANILLA
// MARCHING FRAME).  The vanilla scene is one fitted scene whose density depends on the position alone and which has no
// outside-sphere half, so the grid, the stop rule and the windowed march of the NeO-360 frame (occupancy.hip, march.hip,
// accelerate.hip) apply at face value.  What this file adds to them:
//
//   vm_keep_point   the BOX KEEP RULE: the cell of x = o + t d in a grid over a caller-given box [lo, hi); a point outside the box
//                   is kept (clip == 0) or skipped (clip != 0) - the unit-cube rule clamps, which is not enough here, because
//                   vanilla samples run to `far` whatever the box is;
//   k_vm_keep       the classifier over the CANDIDATES of one launch (below), with the per-workgroup totals of the compaction;
//   k_vm_emit       the second launch of the compaction (occ_rank, occ_points.h): the point rows of the kept candidates;
//   the driver      neo_vanilla_render with the two evaluator launches replaced by the windowed march.
//
// CANDIDATES.  One window (rays r0 .. r0 + rays - 1 of the frame's R), one segment (samples b0 .. b0 + len - 1 of the level's N).
// Candidate p < n len is sample j = b0 + p % len of ray r0 + map[p / len], n = *count alive rays (launch_cull_compact on the running
// transmittance: ascending, the count a device word); map and count NULL: all `rays` rays of the window.  The launches are sized
// for rays x len; a workgroup past the candidates writes a total of 0.  Kept candidates come out in ascending candidate order,
// identically on every run; no atomics, no spinning.
//
// A point row is ONE point (launch_vanilla_mlp*_compact): origin, direction and t of its ray - a vanilla position and its
// direction encoding both come from `viewdirs`, so one direction per row is enough (OccRows' d; v stays unused here) - and
// dst = ray N + j, its place in the level's zero-filled rows.  scatter and advance are march.hip's.
#include "common.h"
#include "ctx.h"
#include "march.h"
#include "occ_points.h"

using namespace neo_host;

// api.hip
int neo_vanilla_eval_compact(neo_ctx* ctx, int slot, const float* rays_o, const float* dirs, const float* t, long cap,
                             const int* count_dev, float* out, hipStream_t s);
int neo_vanilla_eval_dense(neo_ctx* ctx, int slot, const float* rays_o, const float* dirs, const float* t, int t_row_stride, int R,
                           int N, float* out, hipStream_t s);

namespace neo {

namespace {

// VmBox and vm_keep_point, the BOX KEEP RULE of one point: occ_points.h (shared with vanilla_train_march.hip)

// sample and ray of candidate p
__device__ __forceinline__ void vm_candidate(int p, const int* __restrict__ map, int r0, int b0, int len, int& ray, int& j) {
    const int kk = p / len;
    j = b0 + (p - kk * len);
    ray = r0 + (map ? map[kk] : kk);
}

// keep[p] for every candidate; totals (may be null: the mask alone) = kept candidates per workgroup
__global__ __launch_bounds__(OCC_BLOCK) void k_vm_keep(const float* __restrict__ rays_o, const float* __restrict__ dirs,
                                                       const float* __restrict__ t, long stride, const int* __restrict__ map,
                                                       const int* __restrict__ count, int r0, int rays, int b0, int len, VmBox box,
                                                       uint8_t* __restrict__ keep, int* __restrict__ totals) {
    __shared__ int s_seg[OCC_SEGS];
    const int cand = (count ? min(*count, rays) : rays) * len;
    bool k[OCC_ROUNDS];
#pragma unroll
    for (int it = 0; it < OCC_ROUNDS; ++it) {
        const int p = blockIdx.x * OCC_POINTS + it * OCC_BLOCK + threadIdx.x;
        k[it] = false;
        if (p < cand) {
            int ray, j;
            vm_candidate(p, map, r0, b0, len, ray, j);
            k[it] = vm_keep_point(box, rays_o + (long)ray * 3, dirs + (long)ray * 3, t[(long)ray * stride + j]);
            keep[p] = k[it] ? 1 : 0;
        }
    }
    if (totals) occ_total(k, s_seg, totals);
}

__global__ __launch_bounds__(OCC_BLOCK) void k_vm_emit(const float* __restrict__ rays_o, const float* __restrict__ dirs,
                                                       const float* __restrict__ t, long stride, const int* __restrict__ map,
                                                       const int* __restrict__ count, const uint8_t* __restrict__ keep, int r0,
                                                       int rays, int N, int b0, int len, const int* __restrict__ totals,
                                                       float* __restrict__ c_o, float* __restrict__ c_d, float* __restrict__ c_t,
                                                       int* __restrict__ dst, int* __restrict__ rows,
                                                       long long* __restrict__ kept_sum) {
    __shared__ int s_part[OCC_BLOCK / 64];
    __shared__ int s_seg[OCC_SEGS];
    const int cand = (count ? min(*count, rays) : rays) * len;
    const OccRank rk = occ_rank(keep, cand, totals, s_part, s_seg);
#pragma unroll
    for (int it = 0; it < OCC_ROUNDS; ++it) {
        if (!rk.kept[it]) continue;
        const int p = blockIdx.x * OCC_POINTS + it * OCC_BLOCK + threadIdx.x;
        const int k = rk.k[it];
        int ray, j;
        vm_candidate(p, map, r0, b0, len, ray, j);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c_o[(long)k * 3 + a] = rays_o[(long)ray * 3 + a];
            c_d[(long)k * 3 + a] = dirs[(long)ray * 3 + a];
        }
        c_t[k] = t[(long)ray * stride + j];
        dst[k] = ray * N + j;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        *rows = rk.upto;
        if (kept_sum) *kept_sum = *kept_sum + (long long)rk.upto;
    }
}

// the mask of dense (R, N) rows (stride 0: one shared row of positions)
void launch_vm_keep(const float* rays_o, const float* dirs, const float* t, long stride, int R, int N, const VmBox& box, uint8_t* keep,
                    hipStream_t s) {
    const long P = (long)R * N;
    if (P <= 0) return;
    hipLaunchKernelGGL(k_vm_keep, dim3(occ_blocks(P)), dim3(OCC_BLOCK), 0, s, rays_o, dirs, t, stride, (const int*)nullptr,
                       (const int*)nullptr, 0, R, 0, N, box, keep, (int*)nullptr);
}

// classify + compact the candidates of one window and segment: keep (rays x len bytes), w.totals, the point rows and *w.count
void launch_vm_compact(const float* rays_o, const float* dirs, const float* t, long stride, const int* map, const int* count, int r0,
                       int rays, int N, int b0, int len, const VmBox& box, uint8_t* keep, const OccRows& w, long long* kept_sum,
                       hipStream_t s) {
    const long P = (long)rays * len;
    if (P <= 0) return;
    const int nb = occ_blocks(P);
    hipLaunchKernelGGL(k_vm_keep, dim3(nb), dim3(OCC_BLOCK), 0, s, rays_o, dirs, t, stride, map, count, r0, rays, b0, len, box, keep,
                       w.totals);
    hipLaunchKernelGGL(k_vm_emit, dim3(nb), dim3(OCC_BLOCK), 0, s, rays_o, dirs, t, stride, map, count, (const uint8_t*)keep, r0, rays,
                       N, b0, len, (const int*)w.totals, w.o, w.d, w.t, w.dst, w.count, kept_sum);
}

}  // namespace

}  // namespace neo

namespace {

constexpr int VM_WINDOW_DEFAULT = 8192;      // rays per window: 36 MB of point rows at a segment of 64

using neo::vm_box_from;            // occ_points.h
using neo::vm_resolution_ok;

// Per-ray state of one level's march in W[4]: [carry fp64 R | alive fp32 R | stop int R | the alive compaction of one window | one
// keep byte per candidate of one launch].  alive is what the compaction reads: 1 in front of segment 0, then the transmittance.
struct VmState {
    double* carry;
    float* alive;
    int *stop, *cws;
    uint8_t* keep;
    static size_t bytes(size_t r, int win, size_t candidates) { return r * 16 + neo::cull_ws_ints(win) * sizeof(int) + candidates; }
    void carve(void* base, size_t r, int win) {
        carry = static_cast<double*>(base);
        alive = reinterpret_cast<float*>(carry + r);
        stop = reinterpret_cast<int*>(alive + r);
        cws = stop + r;
        keep = reinterpret_cast<uint8_t*>(cws + neo::cull_ws_ints(win));
    }
};

// One level into `out` (R,N,4).  follow: the level obeys the MODE-0 STOP RULE in segments of `segment`; otherwise it is ONE segment
// of N samples and stop = N.  box (may be null): the BOX KEEP RULE.  With neither it is the dense launch of neo_vanilla_render.
// Per window and segment: compact the alive rays, classify + compact (or emit) their samples of the segment, ONE compact evaluator
// launch on single points, scatter into the zero-filled rows, advance - the structure of tp_eval_march (api_tp.hip).
int vm_eval_level(neo_ctx* ctx, hipStream_t s, int level, const float* rays_o, const float* viewdirs, const float* rays_d, int R, int N,
                  const float* pos, long stride, float* out, bool follow, const neo::VmBox* box, float eps, int segment, int win,
                  const VmState& st, int* stop, long long* kept) {
    if (!follow && !box) {
        neo::launch_march_init(nullptr, nullptr, nullptr, R, nullptr, nullptr, nullptr, stop, N, kept, N, s);
        return neo_vanilla_eval_dense(ctx, level, rays_o, viewdirs, pos, static_cast<int>(stride), R, N, out, s);
    }
    const int seg = follow ? std::min(segment, N) : N;
    const size_t cap = static_cast<size_t>(win) * seg;
    if (ctx->ws[5].reserve(neo::occ_rows_bytes(cap))) return NEO_ERR_NOMEM;
    neo::OccRows w;
    w.carve(ctx->ws[5].p, cap);
    HIP_TRY(hipMemsetAsync(out, 0, static_cast<size_t>(R) * N * 16, s));
    neo::launch_march_init(nullptr, nullptr, nullptr, R, nullptr, st.alive, nullptr, stop, follow ? 0 : N, kept, 0, s);
    for (int k0 = 0; k0 < R; k0 += win) {
        const int rows = std::min(win, R - k0);
        for (int b0 = 0; b0 < N; b0 += seg) {
            const int len = std::min(seg, N - b0);
            const long P = static_cast<long>(rows) * len;
            const int *map_w = nullptr, *count_w = nullptr;
            if (follow) {
                neo::launch_cull_compact(st.alive + k0, st.alive + k0, rows, eps, st.cws, nullptr, s);
                map_w = neo::cull_map_of(st.cws, rows);      // the workspace's layout follows the window's row count
                count_w = neo::cull_count_of(st.cws, rows);
            }
            if (box)
                neo::launch_vm_compact(rays_o, viewdirs, pos, stride, map_w, count_w, k0, rows, N, b0, len, *box, st.keep, w, kept, s);
            else      // no Q1 quirk here: the row's own direction is c_d, the view-direction column stays unread (chunk = R keeps it in bounds)
                neo::launch_march_emit(rays_o, viewdirs, viewdirs, nullptr, pos, stride, nullptr, map_w, count_w, k0, rows, R, N, b0, len,
                                       R, w, kept, s);
            if (int rc = neo_vanilla_eval_compact(ctx, level, w.o, w.d, w.t, P, w.count, w.out, s)) return rc;
            neo::launch_march_scatter(w, P, out, s);
            if (follow)
                neo::launch_march_advance_mode(0, out, pos, stride, rays_d, nullptr, nullptr, N, b0, b0 + len, segment, eps, map_w, count_w,
                                               rows, k0, st.carry, nullptr, st.alive, stop, s);
        }
    }
    return NEO_OK;
}

}  // namespace

extern "C" {

// copies into context-owned memory that the frame calls read: an exclusive call, ordered across streams
int neo_vanilla_set_occupancy(neo_ctx* ctx, const uint32_t* bits, int G, const float* lo, const float* hi, int clip, void* stream) {
    ENTER(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    ORDERED(ctx, s);
    if (!bits) {
        ctx->vocc_G = 0;
        return NEO_OK;
    }
    REQUIRE(vm_resolution_ok(G), "occupancy resolution must be 8, 16 or a multiple of 32 in [32, 256]");
    REQUIRE(lo && hi, "null pointer");
    neo::VmBox box{};
    if (const char* msg = vm_box_from(G, lo, hi, box)) return fail(NEO_ERR_INVALID, "%s", msg);
    const size_t bytes = static_cast<size_t>(G) * G * G / 8;
    ctx->vocc_G = 0;
    if (ctx->vocc_bits.reserve(bytes)) return NEO_ERR_NOMEM;
    HIP_TRY(hipMemcpyAsync(ctx->vocc_bits.p, bits, bytes, hipMemcpyDeviceToDevice, s));
    for (int a = 0; a < 3; ++a) {
        ctx->vocc_lo[a] = box.lo[a];
        ctx->vocc_scale[a] = box.scale[a];
    }
    ctx->vocc_clip = clip != 0;
    ctx->vocc_G = G;
    return NEO_OK;
}

int neo_vanilla_set_march_window(neo_ctx* ctx, int rays) {
    ENTER(ctx);
    REQUIRE(rays >= 0 && rays <= 65536, "march window must be 0 (the default) or 1 .. 65536 rays");
    ctx->vanilla_window = rays;
    return NEO_OK;
}

// the pure function k_vm_keep on caller rows; touches no context-owned memory: no ordering scope (as neo_tp_occupancy_keep)
int neo_vanilla_occupancy_keep(neo_ctx* ctx, const uint32_t* bits, int G, const float* lo, const float* hi, int clip,
                               const float* rays_o, const float* dirs, const float* t, int R, int N, uint8_t* keep, void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0 && N >= 1, "bad shape");
    REQUIRE(static_cast<long>(R) * N <= 2147483647L - 1024, "too many points for 32-bit indices");
    neo::VmBox box{};
    if (bits) {
        REQUIRE(vm_resolution_ok(G), "occupancy resolution must be 8, 16 or a multiple of 32 in [32, 256]");
        REQUIRE(lo && hi, "null pointer");
        if (const char* msg = vm_box_from(G, lo, hi, box)) return fail(NEO_ERR_INVALID, "%s", msg);
        box.bits = bits, box.G = G, box.clip = clip != 0;
    }
    if (R == 0) return NEO_OK;
    REQUIRE(rays_o && dirs && t && keep, "null pointer");
    neo::launch_vm_keep(rays_o, dirs, t, N, R, N, box, keep, static_cast<hipStream_t>(stream));
    return check_launch();
}

int neo_vanilla_render_marching(neo_ctx* ctx, const float* rays_o, const float* viewdirs, const float* rays_d, int R, float near,
                                float far, int n_coarse, int n_fine, int white_bkgd, float eps, int segment, int coarse, int use_grid,
                                float* rgb0, float* acc0, float* depth0, float* rgb1, float* acc1, float* depth1,
                                const neo_vanilla_march_samples* samples0, const neo_vanilla_march_samples* samples1, long long* kept,
                                void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0, "negative ray count");
    REQUIRE(n_coarse >= 3 && n_coarse <= 256 && n_fine >= 1 && n_coarse + 1 + n_fine <= 1024, "unsupported sample counts");
    REQUIRE(eps >= 0.0f && eps < 1.0f, "eps must lie in [0, 1)");
    REQUIRE(segment >= 64 && segment % 64 == 0, "segment must be a positive multiple of 64");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (R == 0) {
        if (kept) HIP_TRY(hipMemsetAsync(kept, 0, 2 * sizeof(long long), s));
        return NEO_OK;
    }
    REQUIRE(rays_o && viewdirs && rays_d, "null pointer");
    const int N0 = n_coarse + 1, N1 = N0 + n_fine;
    REQUIRE(static_cast<long>(R) * N1 <= 2147483647L - 1024, "too many points for 32-bit indices");
    const float* t0 = ctx->get_edges(n_coarse, near, far, s);
    const float* u = ctx->get_quantiles(n_fine, s);
    if (!t0 || !u) return fail(NEO_ERR_HIP, "constant table upload failed");
    ORDERED_LANE(ctx, s);      // writes this lane's workspaces only, reads the packed weights and the grid
    const int win = std::min(ctx->vanilla_window > 0 ? ctx->vanilla_window : VM_WINDOW_DEFAULT, R);
    const size_t r = static_cast<size_t>(R);
    neo::VmBox box{};
    const bool grid = use_grid != 0 && ctx->vocc_G != 0;
    if (grid) {
        box.bits = ctx->vocc_bits.as<uint32_t>(), box.G = ctx->vocc_G, box.clip = ctx->vocc_clip;
        for (int a = 0; a < 3; ++a) box.lo[a] = ctx->vocc_lo[a], box.scale[a] = ctx->vocc_scale[a];
    }
    // eps == 0 stops nothing (a transmittance is >= 0 or NaN): no level follows the rule, stop = N
    const bool follow[2] = {coarse != 0 && eps > 0.0f, eps > 0.0f};
    const size_t candidates = grid ? static_cast<size_t>(win) * N1 : 0;
    if (ctx->ws[0].reserve(r * N0 * 16) || ctx->ws[1].reserve(r * N0 * 4) || ctx->ws[2].reserve(r * N1 * 4) ||
        ctx->ws[3].reserve(r * N1 * 16) || ctx->ws[4].reserve(VmState::bytes(r, win, candidates)))
        return NEO_ERR_NOMEM;
    VmState st;
    st.carve(ctx->ws[4].p, r, win);
    float* out0 = samples0 && samples0->rows ? samples0->rows : ctx->ws[0].as<float>();
    float* w0 = samples0 && samples0->w ? samples0->w : ctx->ws[1].as<float>();
    float* t1 = samples1 && samples1->t ? samples1->t : ctx->ws[2].as<float>();
    float* out1 = samples1 && samples1->rows ? samples1->rows : ctx->ws[3].as<float>();
    int* stop0 = samples0 && samples0->stop ? samples0->stop : st.stop;
    int* stop1 = samples1 && samples1->stop ? samples1->stop : st.stop;
    // level 0: one shared row of positions (stride 0); samples along viewdirs (vanilla_nerf/model.py:158-167)
    if (int rc = vm_eval_level(ctx, s, 0, rays_o, viewdirs, rays_d, R, N0, t0, 0, out0, follow[0], grid ? &box : nullptr, eps, segment, win,
                               st, stop0, kept))
        return rc;
    neo::launch_composite(0, out0, t0, 0, rays_d, nullptr, R, N0, white_bkgd, rgb0, acc0, depth0, w0, nullptr, s);
    if (neo::launch_resample(t0, 0, w0, u, 0, R, N0, n_fine, 0, t1, s)) return fail(NEO_ERR_INVALID, "unsupported sample counts");
    if (int rc = vm_eval_level(ctx, s, 1, rays_o, viewdirs, rays_d, R, N1, t1, N1, out1, follow[1], grid ? &box : nullptr, eps, segment,
                               win, st, stop1, kept ? kept + 1 : nullptr))
        return rc;
    neo::launch_composite(0, out1, t1, N1, rays_d, nullptr, R, N1, white_bkgd, rgb1, acc1, depth1, samples1 ? samples1->w : nullptr,
                          nullptr, s);
    if (samples0 && samples0->t) HIP_TRY(hipMemcpyAsync(samples0->t, t0, static_cast<size_t>(N0) * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (samples0 && samples0->keep) neo::launch_vm_keep(rays_o, viewdirs, t0, 0, R, N0, box, samples0->keep, s);
    if (samples1 && samples1->keep) neo::launch_vm_keep(rays_o, viewdirs, t1, N1, R, N1, box, samples1->keep, s);
    return check_launch();
}

}  // extern "C"
