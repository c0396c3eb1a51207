// Empty-space skipping and early ray termination of the VANILLA frame (neo_vanilla_render_marching; include/neo360_hip.h: VANILLA
// MARCHING FRAME).  The vanilla scene is one fitted scene whose density depends on the position alone and which has no
// outside-sphere half, so the grid, the stop rule and the windowed march of the NeO-360 frame apply at face value: this file is
// neo_vanilla_render with the two evaluator launches replaced by march_level (march.h) in composite mode 0.  What differs from the
// NeO-360 users of that loop is data: the grid lies over a caller-given box [lo, hi), outside of which a point is kept (clip == 0)
// or skipped (clip != 0) - the unit cube clamps, which is not enough here, because vanilla samples run to `far` whatever the box
// is; and a vanilla position and its direction encoding both come from `viewdirs`, so one direction per point row is enough
// (OccRows' d; the view column stays unwritten).
#include "common.h"
#include "ctx.h"
#include "march.h"

using namespace neo_host;

// api.hip
int neo_vanilla_eval_compact(neo_ctx* ctx, int slot, const float* rays_o, const float* dirs, const float* t, long cap,
                             const int* count_dev, float* out, hipStream_t s);
int neo_vanilla_eval_dense(neo_ctx* ctx, int slot, const float* rays_o, const float* dirs, const float* t, int t_row_stride, int R,
                           int N, float* out, hipStream_t s);

namespace {

constexpr int VM_WINDOW_DEFAULT = 8192;      // rays per window: 36 MB of point rows at a segment of 64

// One level into `out` (R,N,4) with its stops in st.stop.  Neither a grid nor a rule to follow: the dense launch of
// neo_vanilla_render; otherwise march_level on the level's positions (src.pos / stride / N) with the point rows in W[5].
int vm_eval_level(neo_ctx* ctx, hipStream_t s, int level, const neo::PointSource& src, const neo::OccGrid* grid, const MarchRule& rule,
                  const MarchState& st, int win, float* out, long long* kept) {
    if (!rule.follow && !grid) {
        neo::launch_march_init(nullptr, nullptr, nullptr, src.R, nullptr, nullptr, nullptr, st.stop, src.N, kept, src.N, s);
        return neo_vanilla_eval_dense(ctx, level, src.rays_o, src.dirs, src.pos, static_cast<int>(src.stride), src.R, src.N, out, s);
    }
    const size_t cap = march_level_cap(rule, src.N, win);
    if (ctx->ws[5].reserve(neo::occ_rows_bytes(cap))) return NEO_ERR_NOMEM;
    neo::OccRows w;
    w.carve(ctx->ws[5].p, cap);
    return march_level(src, grid, rule, st, win, w, out, kept, s, [&](const neo::OccRows& rows, long P) {
        return neo_vanilla_eval_compact(ctx, level, rows.o, rows.d, rows.t, P, rows.count, rows.out, s);
    });
}

}  // namespace

extern "C" {

int neo_vanilla_set_march_window(neo_ctx* ctx, int rays) {
    ENTER(ctx);
    REQUIRE(rays >= 0 && rays <= 65536, "march window must be 0 (the default) or 1 .. 65536 rays");
    ctx->vanilla_window = rays;
    return NEO_OK;
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
    const neo::OccGrid* grid = use_grid != 0 ? ctx->vocc.get() : nullptr;
    // eps == 0 stops nothing (a transmittance is >= 0 or NaN): no level follows the rule, stop = N
    const bool follow[2] = {coarse != 0 && eps > 0.0f, eps > 0.0f};
    const size_t candidates = grid ? static_cast<size_t>(win) * N1 : 0;
    if (ctx->ws[0].reserve(r * N0 * 16) || ctx->ws[1].reserve(r * N0 * 4) || ctx->ws[2].reserve(r * N1 * 4) ||
        ctx->ws[3].reserve(r * N1 * 16) || ctx->ws[4].reserve(MarchState::bytes(false, r, win, candidates)))
        return NEO_ERR_NOMEM;
    MarchState st[2];
    st[0].carve(ctx->ws[4].p, false, r, win);
    st[1] = st[0];
    if (samples0 && samples0->stop) st[0].stop = samples0->stop;
    if (samples1 && samples1->stop) st[1].stop = samples1->stop;
    float* out0 = samples0 && samples0->rows ? samples0->rows : ctx->ws[0].as<float>();
    float* w0 = samples0 && samples0->w ? samples0->w : ctx->ws[1].as<float>();
    float* t1 = samples1 && samples1->t ? samples1->t : ctx->ws[2].as<float>();
    float* out1 = samples1 && samples1->rows ? samples1->rows : ctx->ws[3].as<float>();
    // samples along viewdirs (vanilla_nerf/model.py:158-167); level 0: one shared row of positions (stride 0)
    neo::PointSource src{};
    src.rays_o = rays_o, src.dirs = viewdirs, src.R = R;
    const auto rule = [&](int level) { return MarchRule{follow[level], eps, segment, 0, rays_d, nullptr, nullptr, nullptr}; };
    src.pos = t0, src.stride = 0, src.N = N0;
    if (int rc = vm_eval_level(ctx, s, 0, src, grid, rule(0), st[0], win, out0, kept)) return rc;
    neo::launch_composite(0, out0, t0, 0, rays_d, nullptr, R, N0, white_bkgd, rgb0, acc0, depth0, w0, nullptr, s);
    if (neo::launch_resample(t0, 0, w0, u, 0, R, N0, n_fine, 0, t1, s)) return fail(NEO_ERR_INVALID, "unsupported sample counts");
    src.pos = t1, src.stride = N1, src.N = N1;
    if (int rc = vm_eval_level(ctx, s, 1, src, grid, rule(1), st[1], win, out1, kept ? kept + 1 : nullptr)) return rc;
    neo::launch_composite(0, out1, t1, N1, rays_d, nullptr, R, N1, white_bkgd, rgb1, acc1, depth1, samples1 ? samples1->w : nullptr,
                          nullptr, s);
    if (samples0 && samples0->t) HIP_TRY(hipMemcpyAsync(samples0->t, t0, static_cast<size_t>(N0) * sizeof(float), hipMemcpyDeviceToDevice, s));
    // the keep masks of the whole rows, behind the stops as well (no grid: all ones)
    const neo::OccGrid mask_grid = grid ? *grid : neo::OccGrid{};
    if (samples0 && samples0->keep)
        neo::launch_point_keep(neo::point_source_dense(rays_o, viewdirs, t0, 0, R, N0), mask_grid, samples0->keep, nullptr, s);
    if (samples1 && samples1->keep)
        neo::launch_point_keep(neo::point_source_dense(rays_o, viewdirs, t1, N1, R, N1), mask_grid, samples1->keep, nullptr, s);
    return check_launch();
}

}  // extern "C"
