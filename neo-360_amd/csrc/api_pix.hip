// PixelNeRF baseline decoder entry points of the C ABI (models/vanilla_nerf/model_pixel.py:133-258).
#include "common.h"
#include "ctx.h"
#include "march.h"

using namespace neo_host;

namespace {

// algorithmic MACs (model_pixel.py:35-131): per point-view 575*128 + 3*128^2 + 128^2 (bottleneck) + 155*128 =
// 158,976; per point density 128 + 128*128 + rgb 384 = 16,896
double pix_flop_per_point(int nv) { return 2.0 * (nv * 158976.0 + 16896.0); }

// What surrounds a launch of slot `slot`, dense or compact: the slot's state, and in the split arithmetic the one-time range
// guards and the lazy pre-projection (proj: the map to gather, null without pre-projection or in the exact arithmetic)
int pix_prepare(neo_ctx* ctx, int slot, const neo::TpScene& sc, hipStream_t s, const float** proj) {
    MlpSlot& sl = ctx->pix[slot];
    *proj = nullptr;
    if (!sl.ready) return fail(NEO_ERR_STATE, "PixelNeRF MLP slot %d has no weights", slot);
    if (ctx->precision != 1) return NEO_OK;
    // low end: the bottleneck (upload index 6) is folded into view layer 0 in fp64 at pack time (launch_pix_pack_h)
    guard_split_weights(sl, sl.wpack_h.p, neo::pix_wpack_h_bytes(), ctx->flags, s, neo::SPLIT_WEIGHT_LOW_PIX, 1u << 6);
    if (!ctx->pix_latent_checked) {
        neo::launch_f32_range_check(sc.latent, static_cast<size_t>(sc.nv) * sc.Hf * sc.Wf * 512, 65504.0f, ctx->flags, s);
        ctx->pix_latent_checked = true;
    }
    if (!ctx->pix_preproject && !ctx->pix_latent_low_checked) {      // the raw latent is split only without the fp32 pre-projection
        if (int rc = ctx->touch_shared(s)) return rc;
        if (int rc = guard_map_low(ctx, MAP_MAX_PIX_LATENT, &sc.latent, 1, static_cast<size_t>(sc.nv) * sc.Hf * sc.Wf * 512,
                                   neo::SPLIT_MAP_LOW, true, s)) return rc;
        ctx->pix_latent_low_checked = true;
    }
    if (ctx->pix_preproject) {
        // latent pre-projected through this slot's pts_linears.0 latent columns (exact fp32 MFMA): rebuilt only when the
        // scene or the slot's weights changed since the last launch
        if (sl.proj_weights != sl.weights_epoch || sl.proj_scene != ctx->pix_scene_epoch) {
            if (int rc = ctx->touch_shared(s)) return rc;          // shared by both scratch lanes
            const long texels = static_cast<long>(sc.nv) * sc.Hf * sc.Wf;
            if (sl.proj.reserve(static_cast<size_t>(texels) * 512)) return NEO_ERR_NOMEM;
            neo::launch_tp_preproject(sc.latent, texels, sl.wpack.as<float>(), neo::pix_kc_x(), sl.proj.as<float>(), s, 128);
            sl.proj_weights = sl.weights_epoch;
            sl.proj_scene = ctx->pix_scene_epoch;
        }
        *proj = sl.proj.as<float>();
    }
    return NEO_OK;
}

int pix_launch(neo_ctx* ctx, int slot, const neo::TpScene& sc, const neo::TpViews& views, const float* rays_o,
               const float* rays_d, const float* viewdirs, const float* tvals, int t_shared, int R, int N, int chunk,
               float* out, hipStream_t s) {
    const float* proj = nullptr;
    if (int rc = pix_prepare(ctx, slot, sc, s, &proj)) return rc;
    MlpSlot& sl = ctx->pix[slot];
    if (ctx->precision != 1) {
        // exact fp32 MFMA, the reference's operation order up to the folded view layer (mlp_pix.hip): what a range-guard retry
        // of the split evaluator lands on
        neo::TpMlpDev mf{sl.wpack.as<float>(), sl.bias_hp.as<float>(), sl.heads.as<float>()};
        ctx->span_kernel_next = 9;
        ctx->span_begin(s);
        neo::launch_pix_mlp(mf, sc, views, rays_o, rays_d, viewdirs, tvals, t_shared, R, N, chunk, out, s);
        ctx->span_end(s, static_cast<double>(R) * N, pix_flop_per_point(sc.nv));
        return NEO_OK;
    }
    neo::TpMlpHDev mh{sl.wpack_h.p, sl.bias.as<float>(), sl.heads.as<float>(), ctx->flags};
    ctx->span_begin(s);
    neo::launch_pix_mlp_h(mh, proj, sc, views, rays_o, rays_d, viewdirs, tvals, t_shared, R, N, chunk, out, s);
    ctx->span_end(s, static_cast<double>(R) * N, pix_flop_per_point(sc.nv));
    return NEO_OK;
}

// The compact launch of slot `slot` (kernels.h: launch_pix_mlp_h_compact): `cap` rows of one point each under the device count.
// The span prices no points: the live count stays on the device, and a span must not price rows that were never evaluated (as
// tp_launch's for a cull_map launch).
int pix_launch_compact(neo_ctx* ctx, int slot, const neo::TpScene& sc, const neo::TpViews& views, const float* rays_o,
                       const float* rays_d, const float* viewdirs, const float* t, long cap, const int* count_dev, float* out,
                       hipStream_t s) {
    const float* proj = nullptr;
    if (int rc = pix_prepare(ctx, slot, sc, s, &proj)) return rc;
    MlpSlot& sl = ctx->pix[slot];
    if (ctx->precision != 1) {
        neo::TpMlpDev mf{sl.wpack.as<float>(), sl.bias_hp.as<float>(), sl.heads.as<float>()};
        ctx->span_kernel_next = 9;
        ctx->span_begin(s);
        neo::launch_pix_mlp_compact(mf, sc, views, rays_o, rays_d, viewdirs, t, cap, count_dev, out, s);
        ctx->span_end(s, 0.0, pix_flop_per_point(sc.nv));
        return NEO_OK;
    }
    neo::TpMlpHDev mh{sl.wpack_h.p, sl.bias.as<float>(), sl.heads.as<float>(), ctx->flags};
    ctx->span_begin(s);
    neo::launch_pix_mlp_h_compact(mh, proj, sc, views, rays_o, rays_d, viewdirs, t, cap, count_dev, out, s);
    ctx->span_end(s, 0.0, pix_flop_per_point(sc.nv));
    return NEO_OK;
}

constexpr int PM_WINDOW_DEFAULT = 16384;      // rays per window of neo_pix_render_marching: measured, DESIGN.md 4.22 (144 MB of point rows at most)

}  // namespace

extern "C" {

int neo_pix_upload_mlp(neo_ctx* ctx, int slot, const float* const* weights, const float* const* biases,
                       void* stream) {
    ENTER(ctx);
    ORDERED(ctx, static_cast<hipStream_t>(stream));      // touches context-owned memory: ordered across streams
    REQUIRE(slot == 0 || slot == 1, "slot must be 0 (coarse_mlp) or 1 (fine_mlp)");
    REQUIRE(weights && biases, "null pointer table");
    for (int i = 0; i < 9; ++i) REQUIRE(weights[i] && biases[i], "null layer pointer");
    MlpSlot& sl = ctx->pix[slot];
    if (sl.wpack_h.reserve(neo::pix_wpack_h_bytes())) return NEO_ERR_NOMEM;
    if (sl.bias.reserve(neo::pix_bias_floats() * sizeof(float))) return NEO_ERR_NOMEM;
    if (sl.heads.reserve(neo::pix_heads_floats() * sizeof(float))) return NEO_ERR_NOMEM;
    if (sl.wpack.reserve(neo::pix_wpack_floats() * sizeof(float))) return NEO_ERR_NOMEM;
    if (sl.fold_ws.reserve(neo::pix_fold_floats() * sizeof(float))) return NEO_ERR_NOMEM;
    if (sl.bias_hp.reserve(neo::pix_bias_floats() * sizeof(float))) return NEO_ERR_NOMEM;
    neo::launch_pix_pack_h(weights, biases, sl.wpack_h.p, sl.bias.as<float>(), sl.heads.as<float>(), sl.fold_ws.as<float>(),
                           static_cast<hipStream_t>(stream));
    // fp32 fragments of the exact evaluator (mlp_pix.hip); the first 64 k-chunks of its first stage are the latent columns of
    // pts_linears.0 that k_tp_preproject multiplies the scene latent with (pre-projection of the split evaluator)
    neo::launch_pix_pack(weights, biases, sl.fold_ws.as<float>(), sl.bias.as<float>(), sl.bias_hp.as<float>(), sl.wpack.as<float>(),
                         static_cast<hipStream_t>(stream));
    {   // element counts in upload order: pts_linears.0..3, views_linear.0, .1, bottleneck, density, rgb
        const size_t counts[9] = {128 * (63 + 512), 128 * 128, 128 * 128, 128 * 128, 128 * (128 + 27), 128 * 128, 128 * 128, 128, 3 * 128};
        if (int rc = record_weight_maxima(sl, weights, counts, 9, static_cast<hipStream_t>(stream))) return rc;
    }
    sl.input_ch = 3;
    sl.weights_epoch += 1;
    sl.ready = true;
    return check_launch();
}

int neo_pix_set_scene(neo_ctx* ctx, const float* latent, int NV, int Cl, int Hf, int Wf, float image_w,
                      float image_h, void* stream) {
    ENTER(ctx);
    ORDERED(ctx, static_cast<hipStream_t>(stream));      // touches context-owned memory: ordered across streams
    REQUIRE(latent, "null pointer");
    REQUIRE(NV >= 1 && NV <= neo::TP_MAX_VIEWS, "1..8 source views supported");
    REQUIRE(Cl == 512, "the latent width is fixed by the reference MLP (512)");
    REQUIRE(Hf >= 2 && Wf >= 2, "feature maps must be at least 2x2");
    REQUIRE(static_cast<long>(NV) * Hf * Wf * 2048 <= 4294967295L, "latent too large for 32-bit byte offsets (NV*Hf*Wf < 2^21 texels)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ctx->pix_latent.reserve(static_cast<size_t>(NV) * Cl * Hf * Wf * 4)) return NEO_ERR_NOMEM;
    neo::launch_channels_last(latent, NV, Cl, Hf, Wf, ctx->pix_latent.as<float>(), s);
    ctx->pix_scene.latent = ctx->pix_latent.as<float>();
    for (int j = 0; j < 3; ++j) ctx->pix_scene.plane[j] = nullptr;     // no tri-planes in this decoder
    ctx->pix_scene.nv = NV;
    ctx->pix_scene.Hf = Hf; ctx->pix_scene.Wf = Wf; ctx->pix_scene.Hp = 2; ctx->pix_scene.Wp = 2;
    // latent_scaling = [Wf,Hf]/([Wf,Hf]-1)*2 ; scale = latent_scaling/image_size (vanilla_nerf/encoder.py index())
    const float wf = static_cast<float>(Wf), hf = static_cast<float>(Hf);
    ctx->pix_scene.sx = ((wf / (wf - 1.0f)) * 2.0f) / image_w;
    ctx->pix_scene.sy = ((hf / (hf - 1.0f)) * 2.0f) / image_h;
    ctx->pix_scene.fy_sign = 1.0f;                                     // model_pixel.py:203 passes (f, f)
    ctx->pix_scene_ready = true;
    ctx->pix_latent_checked = ctx->pix_latent_low_checked = false;
    ctx->pix_scene_epoch += 1;
    return check_launch();
}

int neo_pix_set_preproject(neo_ctx* ctx, int enable) {
    ENTER(ctx);
    ctx->pix_preproject = enable != 0;
    if (!ctx->pix_preproject)
        for (auto& sl : ctx->pix) { sl.proj.release(); sl.proj_weights = sl.proj_scene = 0; }
    return NEO_OK;
}

int neo_pix_mlp(neo_ctx* ctx, int slot, const float* rays_o, const float* rays_d, const float* viewdirs,
                const float* tvals, int R, int N, int chunk, const float* src_poses, int NV, float focal, float cx,
                float cy, float* out, void* stream) {
    ENTER(ctx);
    ORDERED(ctx, static_cast<hipStream_t>(stream));      // touches context-owned memory: ordered across streams
    REQUIRE(slot == 0 || slot == 1, "slot must be 0 or 1");
    REQUIRE(R >= 0 && N >= 1 && chunk >= 1, "bad shape");
    if (R == 0) return NEO_OK;
    REQUIRE(rays_o && rays_d && viewdirs && tvals && src_poses && out, "null pointer");
    if (!ctx->pix_scene_ready) return fail(NEO_ERR_STATE, "scene latent not set (neo_pix_set_scene)");
    REQUIRE(NV == ctx->pix_scene.nv, "NV differs from the uploaded scene");
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto [sc, views] = call_scene(ctx->pix_scene, src_poses, NV, focal, cx, cy);
    const int rc = pix_launch(ctx, slot, sc, views, rays_o, rays_d, viewdirs, tvals, 0, R, N, chunk, out, s);
    if (rc) return rc;
    return check_launch();
}

int neo_pix_render(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                   const float* src_poses, int NV, float focal, float cx, float cy, float near, float far,
                   int n_coarse, int n_fine, int white_bkgd, float* rgb0, float* acc0, float* depth0, float* rgb1,
                   float* acc1, float* depth1, void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0 && chunk >= 1, "bad ray count / chunk");
    REQUIRE(n_coarse >= 3 && n_coarse <= 256 && n_fine >= 1 && n_coarse + 1 + n_fine <= 1024, "unsupported sample counts");
    if (R == 0) return NEO_OK;
    REQUIRE(rays_o && rays_d && viewdirs && src_poses, "null pointer");
    if (!ctx->pix_scene_ready) return fail(NEO_ERR_STATE, "scene latent not set (neo_pix_set_scene)");
    REQUIRE(NV == ctx->pix_scene.nv, "NV differs from the uploaded scene");
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto [sc, views] = call_scene(ctx->pix_scene, src_poses, NV, focal, cx, cy);
    const int N0 = n_coarse + 1, N1 = N0 + n_fine;
    const float* t0 = ctx->get_edges(n_coarse, near, far, s);
    const float* u = ctx->get_quantiles(n_fine, s);
    if (!t0 || !u) return fail(NEO_ERR_HIP, "constant table upload failed");
    ORDERED_LANE(ctx, static_cast<hipStream_t>(stream));      // writes this lane's workspaces only (a lazy pre-projection: touch_shared)
    if (ctx->ws[0].reserve(static_cast<size_t>(R) * N0 * 16)) return NEO_ERR_NOMEM;
    if (ctx->ws[1].reserve(static_cast<size_t>(R) * N0 * 4)) return NEO_ERR_NOMEM;
    if (ctx->ws[2].reserve(static_cast<size_t>(R) * N1 * 4)) return NEO_ERR_NOMEM;
    if (ctx->ws[3].reserve(static_cast<size_t>(R) * N1 * 16)) return NEO_ERR_NOMEM;
    float* out0 = ctx->ws[0].as<float>();
    float* w0 = ctx->ws[1].as<float>();
    float* t1 = ctx->ws[2].as<float>();
    float* out1 = ctx->ws[3].as<float>();
    // level 0: one shared row of sample positions along rays_d (model_pixel.py:183-192; vanilla helper :415-442)
    int rc = pix_launch(ctx, 0, sc, views, rays_o, rays_d, viewdirs, t0, 1, R, N0, chunk, out0, s);
    if (rc) return rc;
    neo::launch_composite(0, out0, t0, 0, rays_d, nullptr, R, N0, white_bkgd, rgb0, acc0, depth0, w0, nullptr, s);
    // level 1: bins = mids(t0), weights[1:-1] (model_pixel.py:195-206); sort-merge
    if (neo::launch_resample(t0, 0, w0, u, 0, R, N0, n_fine, 0, t1, s)) return fail(NEO_ERR_INVALID, "unsupported sample counts");
    rc = pix_launch(ctx, 1, sc, views, rays_o, rays_d, viewdirs, t1, 0, R, N1, chunk, out1, s);
    if (rc) return rc;
    neo::launch_composite(0, out1, t1, N1, rays_d, nullptr, R, N1, white_bkgd, rgb1, acc1, depth1, nullptr, nullptr, s);
    return check_launch();
}

int neo_pix_set_march_window(neo_ctx* ctx, int rays) {
    ENTER(ctx);
    REQUIRE(rays >= 0 && rays <= 65536, "march window must be 0 (the default) or 1 .. 65536 rays");
    ctx->pix_window = rays;
    return NEO_OK;
}

int neo_pix_mlp_compact(neo_ctx* ctx, int slot, const float* rays_o, const float* rays_d, const float* viewdirs, const float* t,
                        int cap, const int* count_dev, const float* src_poses, int NV, float focal, float cx, float cy, float* out,
                        void* stream) {
    ENTER(ctx);
    ORDERED(ctx, static_cast<hipStream_t>(stream));      // touches context-owned memory: ordered across streams
    REQUIRE(slot == 0 || slot == 1, "slot must be 0 or 1");
    REQUIRE(cap >= 0 && cap <= 2147483647 / 4, "bad shape");
    if (cap == 0) return NEO_OK;
    REQUIRE(rays_o && rays_d && viewdirs && t && count_dev && src_poses && out, "null pointer");
    if (!ctx->pix_scene_ready) return fail(NEO_ERR_STATE, "scene latent not set (neo_pix_set_scene)");
    REQUIRE(NV == ctx->pix_scene.nv, "NV differs from the uploaded scene");
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto [sc, views] = call_scene(ctx->pix_scene, src_poses, NV, focal, cx, cy);
    const int rc = pix_launch_compact(ctx, slot, sc, views, rays_o, rays_d, viewdirs, t, cap, count_dev, out, s);
    if (rc) return rc;
    return check_launch();
}

int neo_pix_render_marching(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                            const float* src_poses, int NV, float focal, float cx, float cy, float near, float far, int n_coarse,
                            int n_fine, int white_bkgd, float eps, int segment, int coarse, int use_grid, float* rgb0, float* acc0,
                            float* depth0, float* rgb1, float* acc1, float* depth1, const neo_vanilla_march_samples* samples0,
                            const neo_vanilla_march_samples* samples1, long long* kept, void* stream) {
    ENTER(ctx);
    REQUIRE(chunk >= 1, "bad ray count / chunk");
    neo::TpScene sc{};
    neo::TpViews views{};
    if (R > 0) {      // as neo_pix_render: no rays is a valid call, whatever else is missing
        REQUIRE(viewdirs && src_poses, "null pointer");
        if (!ctx->pix_scene_ready) return fail(NEO_ERR_STATE, "scene latent not set (neo_pix_set_scene)");
        REQUIRE(NV == ctx->pix_scene.nv, "NV differs from the uploaded scene");
        auto [scene, poses] = call_scene(ctx->pix_scene, src_poses, NV, focal, cx, cy);
        sc = scene, views = poses;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // samples along rays_d, seen along the quirk-Q1 ray of the dense launch (model_pixel.py:183-192, :219-222): the view column
    const Mode0Frame f{rays_o, rays_d, viewdirs, rays_d, R, chunk, near, far, n_coarse, n_fine, white_bkgd, eps, segment, coarse,
                       rgb0, acc0, depth0, rgb1, acc1, depth1, samples0, samples1, kept};
    // both callbacks do what pix_launch does around a launch: the range guards and the lazy pre-projection (touch_shared)
    return march_frame_mode0(
        ctx, f, use_grid != 0 ? ctx->pocc.get() : nullptr, ctx->pix_window > 0 ? ctx->pix_window : PM_WINDOW_DEFAULT, s,
        [&](int level, const neo::PointSource& src, float* out) {
            return pix_launch(ctx, level, sc, views, src.rays_o, src.dirs, src.viewdirs, src.pos, src.stride == 0, src.R, src.N, src.chunk,
                              out, s);
        },
        [&](int level, const neo::OccRows& rows, long P) {
            return pix_launch_compact(ctx, level, sc, views, rows.o, rows.d, rows.v, rows.t, P, rows.count, rows.out, s);
        });
}

}  // extern "C"
