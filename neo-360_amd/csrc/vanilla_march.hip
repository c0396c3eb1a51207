// Empty-space skipping and early ray termination of the VANILLA frame (neo_vanilla_render_marching; include/neo360_hip.h: VANILLA
// MARCHING FRAME).  The vanilla scene is one fitted scene whose density depends on the position alone and which has no
// outside-sphere half, so the grid, the stop rule and the windowed march of the NeO-360 frame apply at face value: this file is
// neo_vanilla_render with the two evaluator launches replaced by march_level in composite mode 0 (march.h: march_frame_mode0).  What differs from the
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
    hipStream_t s = static_cast<hipStream_t>(stream);
    // samples along viewdirs (vanilla_nerf/model.py:158-167), which is also what a point is seen along: no view column
    const Mode0Frame f{rays_o, viewdirs, nullptr, rays_d, R, 0, near, far, n_coarse, n_fine, white_bkgd, eps, segment, coarse,
                       rgb0, acc0, depth0, rgb1, acc1, depth1, samples0, samples1, kept};
    return march_frame_mode0(
        ctx, f, use_grid != 0 ? ctx->vocc.get() : nullptr, ctx->vanilla_window > 0 ? ctx->vanilla_window : VM_WINDOW_DEFAULT, s,
        [&](int level, const neo::PointSource& src, float* out) {
            return neo_vanilla_eval_dense(ctx, level, src.rays_o, src.dirs, src.pos, static_cast<int>(src.stride), src.R, src.N, out, s);
        },
        [&](int level, const neo::OccRows& rows, long P) {
            return neo_vanilla_eval_compact(ctx, level, rows.o, rows.d, rows.t, P, rows.count, rows.out, s);
        });
}

}  // extern "C"
