// NeO-360 (NeRF_TP) entry points of the C ABI: weight / scene upload and the
// two-level, two-region render (neo360/model.py:266-581).
#include "march.h"
#include "tp_frame.h"

#include <algorithm>

using namespace neo_host;

namespace {

// algorithmic MACs of NeRFPPMLP (neo360/model.py:37-158): per point-view 255,424 (fg) / 260,800 (bg),
// per point 4,416 (density 128 + 64x64 + rgb 192); SURVEY.md §8a row a13.
double tp_flop_per_point(int input_ch, int nv) {
    const double per_view = input_ch == 3 ? 255424.0 : 260800.0;
    return 2.0 * (nv * per_view + 4416.0);
}

// The maps a slot gathers in pre-projection modes, recomputed (exact fp32 MFMA, k_tp_preproject: ~1 ms per map) only when the
// scene or the slot's weights changed since they were made: the latent through [W0_loc | W3_loc], and - planes = true - the three
// tri-planes through [W0_world | W3_world] (chunks 64..79 of the fp32 fragment stream).  Shared by both arithmetic modes.
int ensure_projections(neo_ctx* ctx, MlpSlot& sl, const neo::TpScene& sc, bool planes, hipStream_t s, long plane_base[3],
                       bool split_guard = false) {
    const long t_lat = static_cast<long>(sc.nv) * sc.Hf * sc.Wf, t_pl = static_cast<long>(sc.nv) * sc.Hp * sc.Wp;
    for (int j = 0; j < 3; ++j) plane_base[j] = t_lat + j * t_pl;
    const size_t need = neo::tp_proj_bytes(t_lat + (planes ? 3 * t_pl : 0)) + neo::tp_proj_pad_bytes();
    REQUIRE(need <= 4294967295UL, "projected maps too large for 32-bit byte offsets");
    if (need > sl.proj.cap) {          // growing re-allocates: everything in the buffer has to be made again
        if (int rc = ctx->touch_shared(s)) return rc;
        if (sl.proj.reserve(need)) return NEO_ERR_NOMEM;
        sl.proj_weights = sl.proj_scene = sl.projpl_weights = sl.projpl_scene = 0;
    }
    if (sl.proj_weights != sl.weights_epoch || sl.proj_scene != ctx->scene_epoch) {
        if (int rc = ctx->touch_shared(s)) return rc;      // shared by both scratch lanes: this call ends as an exclusive one
        neo::launch_tp_preproject(sc.latent, t_lat, sl.wpack.as<float>(), neo::tp_kc_x(sl.input_ch), sl.proj.as<float>(), s);
        // split arithmetic: a projected map is a STATIC operand of the evaluator (its blends are added to the layer-0 / skip
        // pre-activations, whose hi/lo split the epilogue guards) - checked once per (scene, weights) here, so that a latent the
        // fp16 range cannot hold is reported as a static trip (NEO_FLAG_SPLIT_STATIC: the frame API latches to the exact kernels
        // instead of paying a failed split attempt per frame)
        if (split_guard) neo::launch_f32_range_check(sl.proj.as<float>(), static_cast<size_t>(t_lat) * 256, 65504.0f, ctx->flags, s);
        sl.proj_weights = sl.weights_epoch;
        sl.proj_scene = ctx->scene_epoch;
    }
    if (planes && (sl.projpl_weights != sl.weights_epoch || sl.projpl_scene != ctx->scene_epoch)) {
        if (int rc = ctx->touch_shared(s)) return rc;
        for (int j = 0; j < 3; ++j)
            neo::launch_tp_preproject(sc.plane[j], t_pl, sl.wpack.as<float>(), neo::tp_kc_x(sl.input_ch),
                                      sl.proj.as<float>() + plane_base[j] * 256, s, 256, 128, 64);
        if (split_guard)         // the three projected planes are summed before they meet an accumulator
            neo::launch_f32_range_check(sl.proj.as<float>() + plane_base[0] * 256, static_cast<size_t>(3 * t_pl) * 256, 65504.0f / 3.0f, ctx->flags, s);
        sl.projpl_weights = sl.weights_epoch;
        sl.projpl_scene = ctx->scene_epoch;
    }
    return NEO_OK;
}

// Low end of the range guard for the tri-planes on the paths that split them raw (summed over the three maps first, so their
// common maximum counts): once per scene, a static operand (kernels.h SPLIT_MAP_LOW).
int guard_planes_low(neo_ctx* ctx, const neo::TpScene& sc, hipStream_t s) {
    if (ctx->planes_low_checked == ctx->scene_epoch) return NEO_OK;
    if (int rc = ctx->touch_shared(s)) return rc;      // writes the context's map maxima: this call ends as an exclusive one
    if (int rc = guard_map_low(ctx, MAP_MAX_PLANES, sc.plane, 3, static_cast<size_t>(sc.nv) * sc.Hp * sc.Wp * 128, neo::SPLIT_MAP_LOW,
                               true, s)) return rc;
    ctx->planes_low_checked = ctx->scene_epoch;
    return NEO_OK;
}

// one region's evaluator launch in the context's arithmetic mode
// density_only: the caller reads sigma alone (a level-0 launch whose colour and depth nobody asked for).  The pre-projected split
// evaluators then run their density-only instantiation and the per-ray direction sums are not built; the exact-fp32 and the
// raw-latent split evaluators ignore it and compute everything.
int tp_launch(neo_ctx* ctx, MlpSlot& sl, const neo::TpScene& sc, const neo::TpViews& views, const float* rays_o,
              const float* rays_d, const float* viewdirs, const float* tvals, const float* far, int R, int N, int chunk,
              float* out, hipStream_t s, const int* cull_map = nullptr, const int* cull_count = nullptr,
              bool density_only = false) {
    ORDERED(ctx, s);      // context scratch (tp_dirsum, projected maps, ws[]) is shared by all streams
    const int slot_index = static_cast<int>(&sl - ctx->tp);
    // Patch shape of the ray-patch tile order (neo_ctx_set_ray_grid), per region - measured fabric-side bytes per full-frame launch
    // (profiles/r06_ray_patch_order.log): inside the sphere a ray's footprint is ~2 MB of projected texels, so only the nearest
    // neighbours of a ray are still in the XCD's 4 MB L2: 2 x 2 patches (59.8 -> 41.7 GB; 4 x 4: 45.3, 8 x 8: 51.5); outside, where
    // most taps are the zero-weight placeholder, 8 x 8 (11.6 -> 1.8 GB).  $NEO_TP_PATCH = "<log2 w>,<log2 h>" overrides both.
    neo::TpScene scp = sc;
    if (cull_map) {       // compact launch (neo_tp_render_culled, neo_tp_render_objects): rows are map[] entries, no pixel grid behind them
        scp.cull_map = cull_map;
        scp.cull_count = cull_count;
        scp.grid_w = 0;
    }
    if (scp.grid_w > 0) {
        static int epw = -2, eph = -2;
        if (epw == -2) {
            epw = eph = -1;
            if (const char* e = getenv("NEO_TP_PATCH")) (void)sscanf(e, "%d,%d", &epw, &eph);
        }
        scp.grid_pw = epw >= 0 ? epw : (slot_index < 2 ? 1 : 3);
        scp.grid_ph = eph >= 0 ? eph : (slot_index < 2 ? 1 : 3);
        if (scp.grid_w % (1 << scp.grid_pw) != 0) scp.grid_w = 0;
    }
    // Quad order (point_order.h:quad_point), per slot = per region and level: the samples of G consecutive launch-order rays are
    // interleaved, so that the four rows behind one gather instruction are four neighbouring rays at one sample index instead of
    // four samples of one ray, and a tile holds 64 / G samples of G rays.  Under the patch order above a group of four (a quad) is a
    // 2 x 2 pixel patch inside the sphere and four adjacent pixels of a patch row outside, a group of 16 four such patches in a
    // row / two patch rows; without the hint, consecutive rays of the caller.  The defaults are what profiles/quad_order.log
    // measured per launch of the 640 x 480 frame against the ray-major order (its section 3d, G = 4 / 8 / 16: inside coarse
    // -4.6 / -4.9 / -5.4 %, inside fine -2.6 / -3.3 / -4.4 %, outside coarse -3.1 / -4.3 / -5.5 %, outside fine -0.8 / -1.3 / -1.9 %;
    // section 3e, the shipped table: -6.5 / -4.8 / -6.8 / -2.1 %, every slowest launch below the parent's fastest).  The table
    // below is the one place the defaults are stated (DESIGN.md 4.1 repeats it; tests/test_point_order_cpu.py compares the two).
    // neo_ctx_set_tp_quad, then $NEO_TP_QUAD (read once: 0 = ray-major, 1 = quads of four, 4 / 8 / 16 = rays per group), replace
    // them for every slot; a compact launch never takes the order.
    {
        static const int quad_default[4] = {16, 16, 16, 16};      // fg_coarse, fg_fine, bg_coarse, bg_fine
        static int equad = -2;
        if (equad == -2) {
            const char* e = getenv("NEO_TP_QUAD");
            const int v = e ? atoi(e) : -1;
            equad = v == 1 ? 4 : (v == 0 || v == 4 || v == 8 || v == 16) ? v : -1;
        }
        const int forced = ctx->tp_quad >= 0 ? ctx->tp_quad : equad;
        scp.quad = cull_map ? 0 : forced >= 0 ? forced : quad_default[slot_index];
    }
    long plane_base[3] = {0, 0, 0};          // first texel of each projected tri-plane inside sl.proj
    if (ctx->precision == 1) {
        // range guard of the split arithmetic: tri-planes are summed over three maps before they are split
        if (ctx->planes_checked != ctx->scene_epoch) {
            const size_t n = static_cast<size_t>(sc.nv) * sc.Hp * sc.Wp * 128;
            for (int j = 0; j < 3; ++j) neo::launch_f32_range_check(sc.plane[j], n, 65504.0f / 3.0f, ctx->flags, s);
            ctx->planes_checked = ctx->scene_epoch;
        }
        if (ctx->preproject) {
            // mode 2: planes projected for every slot; mode 3 (default): for the two OUTSIDE-sphere slots only.  Outside, most
            // samples leave the tri-plane volume and every source image: the work list of mlp_tp_hpp.hip gathers 6 of 16
            // (row group, map) pairs on average and the world GEMM stage is pure saving (-8 % / -6 % on the fine / coarse
            // launch).  Inside, every map carries weight on almost every row: 24 more 1 KB gather items per tile-view cost
            // more than the GEMM stage they replace (+1..7 %): profiles/r04_tp_hp_experiments.log.
            const bool planes = ctx->preproject == 2 || (ctx->preproject == 3 && slot_index >= 2);
            if (int rc = ensure_projections(ctx, sl, sc, planes, s, plane_base, true)) return rc;
            // low end: the bottleneck (upload index 6) is folded into view layer 0 in fp64 at pack time and is no operand of
            // these fragments; the latent is projected in fp32, the tri-planes are split raw unless this slot projects them too
            guard_split_weights(sl, sl.wpack_hp.p, neo::tp_wpack_hp_bytes(sl.input_ch), ctx->flags, s, neo::SPLIT_WEIGHT_LOW_TP, 1u << 6);
            if (!planes)
                if (int rc = guard_planes_low(ctx, sc, s)) return rc;
            neo::TpMlpHDev mh{sl.wpack_hp.p, sl.bias_hp.as<float>(), sl.heads.as<float>(), ctx->flags};
            // the view-direction encodings enter the MLP only through their mean over the views, and they depend on the
            // ray alone: summed once per ray here instead of once per sample and view inside the evaluator
            // (a compact inside-sphere launch has no density-only instantiation: it runs the full kernel and needs the sums)
            const bool dens = density_only && !(cull_map && sl.input_ch == 3);
            if (ctx->tp_dirsum->reserve(static_cast<size_t>(R) * 32 * sizeof(float))) return NEO_ERR_NOMEM;
            if (!dens) neo::launch_tp_dirsum(viewdirs, R, views, sc.nv, ctx->tp_dirsum->as<float>(), s);
            ctx->span_kernel_next = planes ? 2 : 1;
            ctx->span_begin(s);
            if (planes)
                neo::launch_tp_mlp_hpp(sl.input_ch, mh, sl.proj.as<float>(), plane_base, scp, views, rays_o, rays_d, viewdirs, tvals, far,
                                       R, N, chunk, ctx->flags, out, ctx->tp_dirsum->as<float>(), s, dens);
            else
                neo::launch_tp_mlp_hp(sl.input_ch, mh, sl.proj.as<float>(), scp, views, rays_o, rays_d, viewdirs, tvals, far, R, N,
                                      chunk, ctx->flags, out, ctx->tp_dirsum->as<float>(), s, dens);
        } else {
            guard_split_weights(sl, sl.wpack_h.p, neo::tp_wpack_h_bytes(sl.input_ch), ctx->flags, s, neo::SPLIT_WEIGHT_LOW_TP);
            if (ctx->latent_checked != ctx->scene_epoch) {
                neo::launch_f32_range_check(sc.latent, static_cast<size_t>(sc.nv) * sc.Hf * sc.Wf * 512, 65504.0f, ctx->flags, s);
                ctx->latent_checked = ctx->scene_epoch;
            }
            // k_tp_mlp_h splits the raw latent and the raw summed tri-planes: both are held to the low end as well
            if (int rc = guard_planes_low(ctx, sc, s)) return rc;
            if (ctx->latent_low_checked != ctx->scene_epoch) {
                if (int rc = ctx->touch_shared(s)) return rc;
                if (int rc = guard_map_low(ctx, MAP_MAX_LATENT, &sc.latent, 1, static_cast<size_t>(sc.nv) * sc.Hf * sc.Wf * 512,
                                           neo::SPLIT_MAP_LOW, true, s)) return rc;
                ctx->latent_low_checked = ctx->scene_epoch;
            }
            neo::TpMlpHDev mh{sl.wpack_h.p, sl.bias.as<float>(), sl.heads.as<float>(), ctx->flags};
            ctx->span_kernel_next = 3;
            ctx->span_begin(s);
            neo::launch_tp_mlp_h(sl.input_ch, mh, scp, views, rays_o, rays_d, viewdirs, tvals, far, R, N, chunk, ctx->flags, out, s);
        }
    } else {
        // exact fp32 MFMA; with pre-projection on, the same algorithm as the split default in the reference's arithmetic: the
        // projected maps are gathered and added, their GEMM stages are not executed per point (the matrix work dominates this
        // kernel at 1/16 of the fp16 rate, so the planes are projected in modes 2 AND 3, for every slot)
        neo::TpMlpDev m{sl.wpack.as<float>(), sl.bias.as<float>(), sl.heads.as<float>()};
        const bool planes = ctx->preproject >= 2;
        if (ctx->preproject)
            if (int rc = ensure_projections(ctx, sl, sc, planes, s, plane_base)) return rc;
        const float* pbase = sl.proj.as<float>();
        const neo::TpPlaneProj pp{{pbase + plane_base[0] * 256, pbase + plane_base[1] * 256, pbase + plane_base[2] * 256}};
        if (ctx->preproject) {      // as on the split path: the direction encodings summed over the views once per ray
            if (ctx->tp_dirsum->reserve(static_cast<size_t>(R) * 32 * sizeof(float))) return NEO_ERR_NOMEM;
            neo::launch_tp_dirsum(viewdirs, R, views, sc.nv, ctx->tp_dirsum->as<float>(), s);
        }
        ctx->span_kernel_next = 4;
        ctx->span_begin(s);
        neo::launch_tp_mlp(sl.input_ch, m, scp, views, rays_o, rays_d, viewdirs, tvals, far, R, N, chunk, ctx->flags, out, s,
                           ctx->preproject ? sl.proj.as<float>() : nullptr, planes ? &pp : nullptr,
                           ctx->preproject ? ctx->tp_dirsum->as<float>() : nullptr);
    }
    // a compact launch's row count exists on the device only: its span carries 0 points / 0 flops (duration and kernel id are
    // real), so nothing derived from the spans prices rows that were never evaluated
    ctx->span_end(s, cull_map ? 0.0 : static_cast<double>(R) * N, tp_flop_per_point(sl.input_ch, sc.nv));
    return NEO_OK;
}

// Rays per window of the skipping frame (neo_tp_set_skip_window replaces it).  A window bounds the extra workspace: a compact row
// is 68 B in W[12] and 128 B in the direction-sum table, so 4096 rays x 385 samples are 1.58 M rows = 107 MB + 202 MB, whatever
// the frame's size; the frame's 75 windows per level cost 5 small launches each.
constexpr int SKIP_WINDOW_DEFAULT = 4096;

// One region's evaluation of one level through THE LEVEL LOOP (march_level, march.h; include/neo360_hip.h: KEEP RULE, STOP RULE,
// OUTSIDE STOP RULE) into `out`: the point rows of one launch in W[12], the level's evaluator as ONE compact launch on single points
// per window and segment - R = the launch's rows, N = 1, the identity map, the device count.  rule: how the level stops, and with
// its composite mode the region (1 inside, 2 outside); win: rows per window; st.stop: samples marched per row; *kept: the evaluated
// samples.
//   inside  (map, rule.count, rule.lam NULL): rows are the frame's rays, pos = the level's dense fg_t.  grid (NULL: none is read): only the
//           samples that the KEEP RULE keeps are evaluated and counted.  A skipped sample stays a zero row, which is what the
//           advance and the composite read: the stops are the STOP RULE on the masked rows.  Without `follow` the level is one
//           segment of N samples per window - the skipping frame.
//   outside (map / rule.count: the frame's survivors; rule.lam: the level's dense lambdas; rule.t_far: the far column): rows are the compact background rows of the culled
//           frame, pos row k at pos + k N (level 0: R equal rows).  The survivor count lives on the device, so the windows cover all R
//           rows and every launch behind the count finds no alive row.
int tp_eval_march(neo_ctx* ctx, const TpFrame& f, const TpFrameArgs& a, const MarchRule& rule, int level, const float* pos, int N,
                  float* out, const int* map, const MarchState& st, int win, long long* kept, bool dens, const neo::OccGrid* grid) {
    hipStream_t s = f.s;
    const bool outside = rule.mode == 2;
    const size_t cap = march_level_cap(rule, N, win);
    if (ctx->ws[12].reserve(neo::occ_rows_bytes(cap))) return NEO_ERR_NOMEM;
    neo::OccRows w;
    w.carve(ctx->ws[12].p, cap);
    neo::launch_occ_iota(w.iota, static_cast<int>(cap), s);
    neo::PointSource src{};
    src.rays_o = a.rays_o, src.dirs = a.rays_d, src.viewdirs = a.viewdirs, src.far = outside ? rule.t_far : nullptr;
    src.pos = pos, src.stride = N, src.map = map;
    src.R = a.R, src.N = N, src.chunk = a.chunk;
    return march_level(src, grid, rule, st, win, w, out, kept, s, [&](const neo::OccRows& rows, long P) {
        return tp_launch(ctx, ctx->tp[(outside ? 2 : 0) + level], f.sc, f.views, rows.o, rows.d, rows.v, rows.t,
                         outside ? rows.far : nullptr, static_cast<int>(P), 1, a.chunk, rows.out, s, rows.iota, rows.count, dens);
    });
}

// The inside-sphere evaluation of one level of a skipping frame (tp_render_dense, TpDenseOptions::skip): the march that follows
// no rule, in windows of skip_window rays.  keep: the caller's (R,N) mask of the level, or null: the mask then lives one window at
// a time in W[13].
int tp_eval_skipping(neo_ctx* ctx, const TpFrame& f, const TpFrameArgs& a, int level, const float* fg_t, int N, float* fg_out,
                     uint8_t* keep, long long* kept) {
    const int win = std::min(ctx->skip_window > 0 ? ctx->skip_window : SKIP_WINDOW_DEFAULT, a.R);
    const size_t cap = static_cast<size_t>(win) * N;
    REQUIRE(cap * 3 <= 2147483647UL, "skip window too large for 32-bit indices");
    if (!keep && ctx->ws[13].reserve(cap)) return NEO_ERR_NOMEM;
    MarchState st{};
    st.keep = keep ? keep : ctx->ws[13].as<uint8_t>();
    st.keep_dense = keep != nullptr;
    const neo::OccGrid* grid = ctx->occ.get();
    if (!grid && keep)      // no grid installed: the point list classifies nothing, and the KEEP RULE keeps every point
        HIP_TRY(hipMemsetAsync(keep, 1, static_cast<size_t>(a.R) * N, f.s));
    return tp_eval_march(ctx, f, a, MarchRule{false, 0.0f, 0, 1, a.rays_d, nullptr, nullptr, nullptr}, level, fg_t, N, fg_out, nullptr, st,
                         win, kept, false, grid);
}

// may the level-0 launches of a frame render be density-only?  Yes when the caller takes none of the level's colours or depth
// (fg_acc and bg_lambda are functions of sigma and stay available)
bool level0_sigma_only(const neo_tp_level_out* level0) {
    return !level0 || !(level0->rgb || level0->fg_rgb || level0->bg_rgb || level0->depth);
}

}  // namespace

// one region's evaluator launch for other translation units (api_train.hip)
int neo_tp_eval_region(neo_ctx* ctx, int slot, const neo::TpScene& sc, const neo::TpViews& views, const float* rays_o,
                       const float* rays_d, const float* viewdirs, const float* tvals, const float* far, int R, int N,
                       int chunk, float* out, hipStream_t s) {
    MlpSlot& sl = ctx->tp[slot];
    if (!sl.ready) return fail(NEO_ERR_STATE, "NeRF_TP MLP slot %d has no weights", slot);
    return tp_launch(ctx, sl, sc, views, rays_o, rays_d, viewdirs, tvals, far, R, N, chunk, out, s);
}

namespace neo_host {

// The preamble of every frame entry point (tp_frame.h).  The order of the checks is part of the ABI: it decides which of two bad
// arguments a call reports.
int TpFrame::begin(neo_ctx* c, const TpFrameArgs& a, bool outside, bool use_grid, const Own& own) {
    ctx = c;
    s = static_cast<hipStream_t>(a.stream);
    REQUIRE(a.R >= 0 && a.chunk >= 1, "bad ray count / chunk");
    REQUIRE(!own.after_rays, own.after_rays);
    REQUIRE(a.n_coarse >= 3 && a.n_coarse <= 256 && a.n_fine >= 1 && a.n_coarse + 1 + a.n_fine <= 1024, "unsupported sample counts");
    REQUIRE(!own.after_counts, own.after_counts);
    if (a.R == 0 || own.empty) {
        empty = true;
        return NEO_OK;
    }
    REQUIRE(a.rays_o && a.rays_d && a.viewdirs && a.src_poses && own.ptrs, "null pointer");
    REQUIRE(!own.after_ptrs, own.after_ptrs);
    if (!ctx->scene_ready) return fail(NEO_ERR_STATE, "scene features not set (neo_tp_set_scene)");
    REQUIRE(a.NV == ctx->scene.nv, "NV differs from the uploaded scene");
    for (int i = 0; i < (outside ? 4 : 2); ++i)          // the compact marches do not need the outside-sphere slots 2, 3
        if (!ctx->tp[i].ready) return fail(NEO_ERR_STATE, "NeRF_TP MLP slot %d has no weights", i);
    if (outside)
        REQUIRE(ctx->tp[0].input_ch == 3 && ctx->tp[1].input_ch == 3 && ctx->tp[2].input_ch == 4 && ctx->tp[3].input_ch == 4,
                "slots 0,1 must be fg (input_ch 3), slots 2,3 bg (input_ch 4)");
    else
        REQUIRE(ctx->tp[0].input_ch == 3 && ctx->tp[1].input_ch == 3, "slots 0,1 must be fg (input_ch 3)");
    const CallScene cs = call_scene(ctx->scene, a.src_poses, a.NV, a.focal, a.cx, a.cy);
    sc = cs.sc;
    views = cs.views;
    if (use_grid) {       // pixel-grid hint of the frame API: the evaluators walk the rays in patches; compact launches drop it (tp_launch)
        sc.grid_w = ctx->ray_grid_w;
        sc.grid_first = ctx->ray_grid_first;
    }
    N0 = a.n_coarse + 1;
    N1 = N0 + a.n_fine;
    edges = ctx->get_edges(a.n_coarse, 0.0f, 1.0f, s);     // linspace(0,1,n+1)
    u = ctx->get_quantiles(a.n_fine, s);
    if (!edges || !u) return fail(NEO_ERR_HIP, "constant table upload failed");
    // workspaces: this lane's set (neo_ctx_set_lane); a frame call reads shared weights / maps and writes lane scratch only
    if (int rc = ctx->order_begin(s, true)) return rc;      // ORDERED_LANE, the scope ending with this object
    ordered = true;
    return NEO_OK;
}

// The dense two-level launch list: sphere test, level-0 rows, then per level the two evaluator launches, [edit,] the inside-sphere
// composite [with layers], [decompose,] the outside-sphere composite, merge, [extras,] [sample copies,] and behind level 0 the two
// resamples.  Without options it is neo_tp_render's list with a full level 0: the level-1 composites pass a NULL w_out and
// W[10] / W[11] are not touched.  A level whose extras are asked for has both composites write their weights (level 0
// does so anyway, for the resampling; level 1 into W[10] / W[11]); a level-1 decomposition or a copy of the level-1 scene weights
// needs the inside-sphere ones alone (W[10]).
int tp_render_dense(neo_ctx* ctx, const TpFrameArgs& a, const TpDenseOptions& o) {
    TpFrame::Own own;
    bool want_extras[2];
    for (int l = 0; l < 2; ++l) {
        const neo_tp_extras_out* ex = o.extras[l];
        want_extras[l] = ex && (ex->opacity || ex->disparity || (ex->dist_pct && o.n_u > 0));
        if (!own.after_counts && ex && ex->dist_pct && o.n_u > 0 && !o.u_extras) own.after_counts = "null quantile table";
    }
    if (!(o.n_u >= 0 && o.n_u <= 8)) own.after_counts = "bad quantile count (0 <= n_u <= 8)";
    if (!((o.K_edit == 0 && o.K_dec == 0) || (o.near_inst && o.far_inst))) own.after_ptrs = "null interval pointer";
    else if (!(o.L == 0 || (o.layers && o.layers->key && o.layers->rgb && o.layers->acc && o.layers->depth)))
        own.after_ptrs = "null layer pointer";
    TpFrame f;
    if (int rc = f.begin(ctx, a, true, true, own)) return rc;
    if (f.empty) return NEO_OK;
    hipStream_t s = f.s;
    const int R = a.R, chunk = a.chunk, N0 = f.N0, N1 = f.N1;
    const float *rays_o = a.rays_o, *rays_d = a.rays_d, *viewdirs = a.viewdirs;

    auto* W = ctx->ws;
    const size_t r = static_cast<size_t>(R);
    const bool want_fg_w1 = want_extras[1] || o.decomposed[1] || (o.samples[1] && o.samples[1]->fg_w);
    TpDenseRows rows;
    if (rows.reserve(W, r, N0, N1) || W[9].reserve(r * 16 * 4)) return NEO_ERR_NOMEM;
    if (want_fg_w1 && W[10].reserve(r * N1 * 4)) return NEO_ERR_NOMEM;
    if (want_extras[1] && W[11].reserve(r * N1 * 4)) return NEO_ERR_NOMEM;
    auto [far, fg_t0, bg_s0, fg_out, bg_out, fg_w0, bg_w0, fg_t1, bg_s1] = rows;
    float* fg_w1 = want_fg_w1 ? W[10].as<float>() : nullptr;          // level-1 weights: only the options read them
    float* bg_w1 = want_extras[1] ? W[11].as<float>() : nullptr;
    float* scratch = W[9].as<float>();   // per-ray: fg_rgb(3) fg_depth fg_acc lambda bg_rgb(3) bg_depth
    float* s_fg_rgb = scratch;
    float* s_fg_depth = scratch + r * 3;
    float* s_fg_acc = scratch + r * 4;
    float* s_lambda = scratch + r * 5;
    float* s_bg_rgb = scratch + r * 6;
    float* s_bg_depth = scratch + r * 9;

    neo::launch_sphere(rays_o, rays_d, R, far, nullptr, ctx->flags, s);
    neo::launch_tp_level0(far, f.edges, R, N0, f.near, fg_t0, bg_s0, s);

    // the coarse level feeds the fine one through its weights (sigma) alone: when the caller allows it and nobody reads its colour
    // or depth, its launches are density-only and its composites write neither
    const bool sigma0 = o.level0_may_be_sigma_only && level0_sigma_only(o.level[0]);
    const float* fg_t = fg_t0;
    const float* bg_s = bg_s0;
    for (int level = 0; level < 2; ++level) {
        const int N = level == 0 ? N0 : N1;
        const neo_tp_level_out* lo = o.level[level];
        const neo_tp_edit_samples* so = o.samples[level];
        const neo_tp_decomposed_out* dc = o.decomposed[level];
        const bool dens = level == 0 && sigma0;
        if (o.skip) {
            if (int rc = tp_eval_skipping(ctx, f, a, level, fg_t, N, fg_out, o.fg_keep[level], o.kept ? o.kept + level : nullptr)) return rc;
            if (o.fg_rows[level]) HIP_TRY(hipMemcpyAsync(o.fg_rows[level], fg_out, r * N * 16, hipMemcpyDeviceToDevice, s));
        } else if (int rc = tp_launch(ctx, ctx->tp[level], f.sc, f.views, rays_o, rays_d, viewdirs, fg_t, nullptr, R, N, chunk, fg_out, s, nullptr, nullptr, dens)) return rc;
        if (int rc = tp_launch(ctx, ctx->tp[2 + level], f.sc, f.views, rays_o, rays_d, viewdirs, bg_s, far, R, N, chunk, bg_out, s, nullptr, nullptr, dens)) return rc;
        float* fg_rgb = dens ? nullptr : (lo && lo->fg_rgb) ? lo->fg_rgb : s_fg_rgb;
        float* bg_rgb = dens ? nullptr : (lo && lo->bg_rgb) ? lo->bg_rgb : s_bg_rgb;
        float* fg_acc = (lo && lo->fg_acc) ? lo->fg_acc : s_fg_acc;
        float* lam = (lo && lo->bg_lambda) ? lo->bg_lambda : s_lambda;
        float* fg_w = level == 0 ? fg_w0 : fg_w1;
        float* bg_w = level == 0 ? bg_w0 : bg_w1;
        if (o.K_edit > 0) neo::launch_tp_edit(fg_out, fg_t, o.near_inst, o.far_inst, o.K_edit, R, N, *o.edit, s);
        if (o.L > 0)
            neo::launch_composite_layers(fg_out, fg_t, rays_d, far, R, N, o.layers->key, o.layers->rgb, o.layers->acc, o.layers->depth,
                                         o.L, fg_rgb, fg_acc, dens ? nullptr : s_fg_depth, fg_w, lam, so ? so->visibility : nullptr, s);
        else
            neo::launch_composite(1, fg_out, fg_t, N, rays_d, far, R, N, 0, fg_rgb, fg_acc, dens ? nullptr : s_fg_depth, fg_w, lam, s);
        if (dc)        // rows, positions and scene weights are still in this lane's scratch; bg_lambda is this level's own
            neo::launch_tp_decompose(fg_out, fg_t, fg_w, o.near_inst, o.far_inst, o.K_dec, R, N, lam, dc->rgb, dc->acc, dc->depth, dc->id, s);
        neo::launch_composite(2, bg_out, bg_s, N, nullptr, nullptr, R, N, 0, bg_rgb, nullptr, dens ? nullptr : s_bg_depth, bg_w,
                              nullptr, s);
        if (lo && (lo->rgb || lo->depth))
            neo::launch_tp_merge(fg_rgb, s_fg_depth, lam, bg_rgb, s_bg_depth, R, lo->rgb, lo->depth, s);
        if (want_extras[level]) {
            const neo_tp_extras_out* ex = o.extras[level];
            if (neo::launch_tp_extras(fg_t, fg_w, far, bg_s, bg_w, lam, rays_o, rays_d, R, N, o.u_extras, o.n_u, ex->opacity,
                                      ex->disparity, ex->dist_pct, s))
                return fail(NEO_ERR_INVALID, "unsupported sample or quantile count");
        }
        if (so) {
            const size_t row = r * N * sizeof(float);
            if (so->fg_t) HIP_TRY(hipMemcpyAsync(so->fg_t, fg_t, row, hipMemcpyDeviceToDevice, s));
            if (so->bg_s) HIP_TRY(hipMemcpyAsync(so->bg_s, bg_s, row, hipMemcpyDeviceToDevice, s));
            if (so->fg_w) HIP_TRY(hipMemcpyAsync(so->fg_w, fg_w, row, hipMemcpyDeviceToDevice, s));
        }
        if (level == 0) {
            // hierarchical resampling (model.py:306-332) on the SCENE weights (the fine positions do not depend on layers): fg
            // ascending; bg on the descending inverse radius
            if (neo::launch_resample(fg_t0, N0, fg_w0, f.u, 0, R, N0, a.n_fine, 0, fg_t1, s) ||
                neo::launch_resample(bg_s0, N0, bg_w0, f.u, 0, R, N0, a.n_fine, 1, bg_s1, s))
                return fail(NEO_ERR_INVALID, "unsupported sample counts");
            fg_t = fg_t1;
            bg_s = bg_s1;
        }
    }
    return check_launch();
}

// The compact two-level march (tp_frame.h): the two inside-sphere MLPs on rows that are map[] entries, *count of them.
int tp_march_compact(const TpFrame& f, const TpFrameArgs& a, const TpCompactRows& c, const int* map, const int* count, int white) {
    neo_ctx* ctx = f.ctx;
    hipStream_t s = f.s;
    const int R = a.R, N0 = f.N0, N1 = f.N1;
    if (int rc = tp_launch(ctx, ctx->tp[0], f.sc, f.views, a.rays_o, a.rays_d, a.viewdirs, c.t0, nullptr, R, N0, a.chunk, c.out, s, map, count)) return rc;
    neo::launch_composite(1, c.out, c.t0, N0, c.rays_d, c.far, R, N0, white, c.rgb[0], c.acc[0], c.depth[0], c.w0, nullptr, s, count);
    if (neo::launch_resample(c.t0, N0, c.w0, f.u, 0, R, N0, a.n_fine, 0, c.t1, s, count)) return fail(NEO_ERR_INVALID, "unsupported sample counts");
    if (int rc = tp_launch(ctx, ctx->tp[1], f.sc, f.views, a.rays_o, a.rays_d, a.viewdirs, c.t1, nullptr, R, N1, a.chunk, c.out, s, map, count)) return rc;
    neo::launch_composite(1, c.out, c.t1, N1, c.rays_d, c.far, R, N1, white, c.rgb[1], c.acc[1], c.depth[1], nullptr, nullptr, s, count);
    return NEO_OK;
}

}  // namespace neo_host

extern "C" {

int neo_tp_upload_mlp(neo_ctx* ctx, int slot, int input_ch, const float* const* weights,
                      const float* const* biases, void* stream) {
    ENTER(ctx);
    ORDERED(ctx, static_cast<hipStream_t>(stream));      // touches context-owned memory: ordered across streams
    REQUIRE(slot >= 0 && slot < 4, "slot must be 0..3 (fg_coarse, fg_fine, bg_coarse, bg_fine)");
    REQUIRE(input_ch == 3 || input_ch == 4, "input_ch must be 3 (fg) or 4 (bg)");
    REQUIRE(weights && biases, "null pointer table");
    for (int i = 0; i < 9; ++i) REQUIRE(weights[i] && biases[i], "null layer pointer");
    MlpSlot& sl = ctx->tp[slot];
    if (sl.wpack.reserve(neo::tp_wpack_floats(input_ch) * sizeof(float))) return NEO_ERR_NOMEM;
    if (sl.bias.reserve(neo::tp_bias_floats() * sizeof(float))) return NEO_ERR_NOMEM;
    if (sl.heads.reserve(neo::tp_heads_floats() * sizeof(float))) return NEO_ERR_NOMEM;
    if (sl.wpack_h.reserve(neo::tp_wpack_h_bytes(input_ch))) return NEO_ERR_NOMEM;
    if (sl.wpack_hp.reserve(neo::tp_wpack_hp_bytes(input_ch))) return NEO_ERR_NOMEM;
    if (sl.fold_ws.reserve(neo::tp_fold_floats() * sizeof(float))) return NEO_ERR_NOMEM;
    neo::launch_tp_pack(input_ch, weights, biases, sl.wpack.as<float>(), sl.bias.as<float>(), sl.heads.as<float>(),
                        static_cast<hipStream_t>(stream), sl.fold_ws.as<float>());
    neo::launch_tp_pack_h(input_ch, weights, sl.wpack_h.p, static_cast<hipStream_t>(stream));
    if (sl.bias_hp.reserve(neo::tp_bias_floats() * sizeof(float)) || sl.fold_ws.reserve(neo::tp_fold_floats() * sizeof(float)))
        return NEO_ERR_NOMEM;
    neo::launch_tp_pack_hp(input_ch, weights, biases, sl.wpack_hp.p, sl.fold_ws.as<float>(), sl.bias.as<float>(),
                           sl.bias_hp.as<float>(), static_cast<hipStream_t>(stream));
    {   // element counts in upload order: pts_linears.0..3 (the skip concatenation feeds 3), views_linear.0, .1, bottleneck, density, rgb
        const size_t x = static_cast<size_t>(21 * input_ch + 512 + 128);
        const size_t counts[9] = {128 * x, 128 * 128, 128 * 128, 128 * (128 + x), 64 * (128 + 27), 64 * 64, 128 * 128, 128, 3 * 64};
        if (int rc = record_weight_maxima(sl, weights, counts, 9, static_cast<hipStream_t>(stream))) return rc;
    }
    sl.weights_epoch += 1;
    sl.input_ch = input_ch;
    sl.ready = true;
    return check_launch();
}

int neo_tp_set_scene(neo_ctx* ctx, const float* plane_xz, const float* plane_xy, const float* plane_yz, int NV,
                     int Cw, int Hp, int Wp, const float* latent, int Cl, int Hf, int Wf, float image_w,
                     float image_h, void* stream) {
    ENTER(ctx);
    ORDERED(ctx, static_cast<hipStream_t>(stream));      // touches context-owned memory: ordered across streams
    REQUIRE(plane_xz && plane_xy && plane_yz && latent, "null pointer");
    REQUIRE(NV >= 1 && NV <= neo::TP_MAX_VIEWS, "1..8 source views supported");
    REQUIRE(Cw == 128 && Cl == 512, "feature widths are fixed by the reference MLP (128 world, 512 local)");
    REQUIRE(Hp >= 2 && Wp >= 2 && Hf >= 2 && Wf >= 2, "feature maps must be at least 2x2");
    REQUIRE(static_cast<long>(NV) * Hf * Wf * 2048 <= 4294967295L && static_cast<long>(NV) * Hp * Wp * 512 <= 4294967295L,
            "feature maps too large for 32-bit byte offsets (NV*Hf*Wf < 2^21 texels)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float* planes[3] = {plane_xz, plane_xy, plane_yz};
    for (int j = 0; j < 3; ++j) {
        if (ctx->plane[j].reserve(static_cast<size_t>(NV) * Cw * Hp * Wp * 4)) return NEO_ERR_NOMEM;
        neo::launch_channels_last(planes[j], NV, Cw, Hp, Wp, ctx->plane[j].as<float>(), s);
        ctx->scene.plane[j] = ctx->plane[j].as<float>();
    }
    if (ctx->latent.reserve(static_cast<size_t>(NV) * Cl * Hf * Wf * 4)) return NEO_ERR_NOMEM;
    neo::launch_channels_last(latent, NV, Cl, Hf, Wf, ctx->latent.as<float>(), s);
    ctx->scene.latent = ctx->latent.as<float>();
    ctx->scene.nv = NV;
    ctx->scene.Hf = Hf; ctx->scene.Wf = Wf; ctx->scene.Hp = Hp; ctx->scene.Wp = Wp;
    // latent_scaling = [Wf,Hf]/([Wf,Hf]-1)*2 (encoder_pn.py:204-206); scale = latent_scaling/image_size (:121-123)
    const float wf = static_cast<float>(Wf), hf = static_cast<float>(Hf);
    const float lsx = (wf / (wf - 1.0f)) * 2.0f, lsy = (hf / (hf - 1.0f)) * 2.0f;
    ctx->scene.sx = lsx / image_w;
    ctx->scene.sy = lsy / image_h;
    ctx->scene.fy_sign = -1.0f;                                       // NeRF_TP projects with (f, -f) (model.py:243)
    ctx->scene_epoch += 1;
    ctx->scene_ready = true;
    ctx->occ.clear();      // an occupancy grid describes one scene
    return check_launch();
}

int neo_tp_set_preproject(neo_ctx* ctx, int enable) {
    ENTER(ctx);
    (void)hipDeviceSynchronize();        // projected maps may be released below: nothing of this context may still read them
    REQUIRE(enable >= 0 && enable <= 3, "preproject mode must be 0 (off), 1 (latent), 2 (latent + tri-planes) or 3 (2 except slot 0)");
    ctx->preproject = enable;
    for (auto& sl : ctx->tp) sl.range_checked = 0;       // the other fragment set is checked at its first launch
    if (!ctx->preproject)
        for (auto& sl : ctx->tp) { sl.proj.release(); sl.proj_weights = sl.proj_scene = 0; }
    if (ctx->preproject < 2)
        for (auto& sl : ctx->tp) {           // the plane part goes with the next (smaller) allocation; mark it stale now
            if (ctx->preproject) sl.proj.release();
            sl.proj_weights = sl.proj_scene = sl.projpl_weights = sl.projpl_scene = 0;
        }
    return NEO_OK;
}

int neo_tp_mlp(neo_ctx* ctx, int slot, const float* rays_o, const float* rays_d, const float* viewdirs,
               const float* tvals, const float* far, int R, int N, int chunk, const float* src_poses, int NV,
               float focal, float cx, float cy, float* out, void* stream) {
    ENTER(ctx);
    ORDERED(ctx, static_cast<hipStream_t>(stream));      // touches context-owned memory: ordered across streams
    REQUIRE(slot >= 0 && slot < 4, "slot must be 0..3");
    REQUIRE(R >= 0 && N >= 1 && chunk >= 1, "bad shape");
    if (R == 0) return NEO_OK;
    REQUIRE(rays_o && rays_d && viewdirs && tvals && src_poses && out, "null pointer");
    if (!ctx->scene_ready) return fail(NEO_ERR_STATE, "scene features not set (neo_tp_set_scene)");
    REQUIRE(NV == ctx->scene.nv, "NV differs from the uploaded scene");
    MlpSlot& sl = ctx->tp[slot];
    if (!sl.ready) return fail(NEO_ERR_STATE, "NeRF_TP MLP slot %d has no weights", slot);
    REQUIRE(sl.input_ch == (slot < 2 ? 3 : 4), "slots 0,1 must hold fg weights, 2,3 bg weights");
    REQUIRE(slot < 2 || far, "far required for the outside-sphere slots");
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto [sc, views] = call_scene(ctx->scene, src_poses, NV, focal, cx, cy);
    if (int rc = tp_launch(ctx, sl, sc, views, rays_o, rays_d, viewdirs, tvals, far, R, N, chunk, out, s)) return rc;
    return check_launch();
}

int neo_tp_render(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                  const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse, int n_fine,
                  int white_bkgd, const neo_tp_level_out* level0, const neo_tp_level_out* level1, void* stream) {
    return neo_tp_render_extras(ctx, rays_o, rays_d, viewdirs, R, chunk, src_poses, NV, focal, cx, cy, n_coarse, n_fine, white_bkgd,
                                level0, level1, nullptr, 0, nullptr, nullptr, stream);
}

// neo_tp_render with the extras of tp_extras.hip per level: tp_render_dense with a level 0 that may be density-only.  Without
// extras (both structs NULL or empty) the launch list, the workspaces and every output are neo_tp_render's.
int neo_tp_render_extras(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                         const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse, int n_fine,
                         int white_bkgd, const neo_tp_level_out* level0, const neo_tp_level_out* level1, const float* u_extras,
                         int n_u, const neo_tp_extras_out* extras0, const neo_tp_extras_out* extras1, void* stream) {
    ENTER(ctx);
    (void)white_bkgd;  // out_depth=True semantics: the reference composites with white_bkgd=False (model.py:477-501)
    TpDenseOptions o;
    o.level[0] = level0;
    o.level[1] = level1;
    o.level0_may_be_sigma_only = true;
    o.u_extras = u_extras;
    o.n_u = n_u;
    o.extras[0] = extras0;
    o.extras[1] = extras1;
    return tp_render_dense(ctx, {rays_o, rays_d, viewdirs, R, chunk, src_poses, NV, focal, cx, cy, n_coarse, n_fine, stream}, o);
}

// The dense frame with a full level 0 whose inside-sphere launches skip the samples the installed occupancy grid clears
// (tp_eval_skipping); every other launch of the list is neo_tp_render's.
int neo_tp_render_skipping(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                           const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse, int n_fine,
                           const neo_tp_level_out* level0, const neo_tp_level_out* level1, const neo_tp_skip_samples* samples0,
                           const neo_tp_skip_samples* samples1, long long* kept, void* stream) {
    ENTER(ctx);
    TpDenseOptions o;
    o.level[0] = level0;
    o.level[1] = level1;
    o.skip = true;
    o.kept = kept;
    const neo_tp_skip_samples* given[2] = {samples0, samples1};
    neo_tp_edit_samples rows[2];
    for (int l = 0; l < 2; ++l) {
        if (!given[l]) continue;
        rows[l] = {given[l]->fg_t, given[l]->fg_w, given[l]->bg_s, nullptr};
        o.samples[l] = &rows[l];
        o.fg_keep[l] = given[l]->fg_keep;
        o.fg_rows[l] = given[l]->fg_rows;
    }
    if (kept && R == 0 && chunk >= 1) HIP_TRY(hipMemsetAsync(kept, 0, 2 * sizeof(long long), static_cast<hipStream_t>(stream)));
    return tp_render_dense(ctx, {rays_o, rays_d, viewdirs, R, chunk, src_poses, NV, focal, cx, cy, n_coarse, n_fine, stream}, o);
}

// the pure function of tp_extras.hip on caller rows; touches no context-owned memory: no ordering scope (as neo_mip_extras)
int neo_tp_extras(neo_ctx* ctx, const float* fg_t, const float* fg_w, const float* far, const float* bg_s, const float* bg_w,
                  const float* lambda, const float* rays_o, const float* rays_d, int R, int N, const float* u, int n_u, float* opacity,
                  float* disparity, float* dist_pct, void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0 && N >= 1 && N <= 1024, "bad shape (1 <= N <= 1024)");
    REQUIRE(n_u >= 0 && n_u <= 8, "bad quantile count (0 <= n_u <= 8)");
    REQUIRE((bg_s != nullptr) == (bg_w != nullptr) && (bg_s != nullptr) == (lambda != nullptr),
            "bg_s, bg_w and lambda go together: all three, or none for the inside-only histogram");
    if (R == 0) return NEO_OK;
    REQUIRE(fg_t && fg_w && far && rays_o && rays_d && (u || n_u == 0 || !dist_pct), "null pointer");
    if (neo::launch_tp_extras(fg_t, fg_w, far, bg_s, bg_w, lambda, rays_o, rays_d, R, N, u, n_u, opacity, disparity, dist_pct,
                              static_cast<hipStream_t>(stream)))
        return fail(NEO_ERR_INVALID, "unsupported sample or quantile count");
    return check_launch();
}

// What an entry point asks of tp_render_marching beyond the frame's arguments.
struct TpMarchOptions {
    const char* after_counts;      // the entry point's own eps / segment check (TpFrame::Own), or NULL
    bool stop_inside;              // false (neo_tp_render_culled): no level follows the STOP RULE inside the sphere
    bool use_occ;                  // an installed occupancy grid is read (the KEEP RULE)
    bool outside;                  // the outside-sphere march follows the OUTSIDE STOP RULE
};

// the eps / segment check of the three marching entry points
static const char* march_arg_check(float eps, int segment) {
    if (!(eps >= 0.0f && eps < 1.0f)) return "eps must lie in [0, 1)";
    if (!(segment >= 64 && segment % 64 == 0)) return "segment must be a positive multiple of 64";
    return nullptr;
}

// The one driver of the culled and the marching frames: the foreground of both levels first (nothing in a ray's background half
// feeds its foreground half), then the background on the rays that still let light through (launch_cull_compact on the two
// bg_lambda; grids sized for R, every kernel takes its row count from the device word).
//   stop_inside = false   neo_tp_render_culled: both foreground levels are dense launches with the ray-patch order, the background
//                         is the compact launch; no march state, no point rows (W[12] / W[13] are not touched), no sample copies;
//   stop_inside = true    the inside-sphere march of level 1 - with `coarse` also of level 0 - stops by the STOP RULE (tp_eval_march).
//                         use_occ = false (neo_tp_render_terminating): an installed grid is not read, bits stays NULL.  use_occ =
//                         true (neo_tp_render_accelerated): with a grid installed the marches also obey the KEEP RULE, and a level 0
//                         without `coarse` is tp_eval_skipping.  `outside` (neo_tp_render_marching only): the outside-sphere march of
//                         level 1 - with `coarse` also of level 0 - obeys the OUTSIDE STOP RULE instead of the compact launch.
// kept: int64[2], the inside counters; kept_out (may be NULL): int64[2], the outside ones.  A level that does not march costs only
// what its caller asks for.  The caller has entered the context.
static int tp_render_marching(neo_ctx* ctx, const TpFrameArgs& a, const neo_tp_level_out* level0, const neo_tp_level_out* level1,
                              float eps, int segment, int coarse, const neo_tp_march_samples* samples0,
                              const neo_tp_march_samples* samples1, long long* kept, long long* kept_out, int* survivors_out,
                              const TpMarchOptions& o) {
    const float *rays_o = a.rays_o, *rays_d = a.rays_d, *viewdirs = a.viewdirs;
    const int R = a.R, chunk = a.chunk, n_fine = a.n_fine;
    const bool use_occ = o.use_occ, outside = o.outside;
    TpFrame::Own own;
    own.after_counts = o.after_counts;
    TpFrame f;      // a dense launch keeps the ray-patch order; compact launches drop it (tp_launch)
    if (int rc = f.begin(ctx, a, true, true, own)) return rc;
    hipStream_t s = f.s;
    if (f.empty) {
        if (survivors_out) HIP_TRY(hipMemsetAsync(survivors_out, 0, sizeof(int), s));
        if (kept) HIP_TRY(hipMemsetAsync(kept, 0, 2 * sizeof(long long), s));
        if (kept_out) HIP_TRY(hipMemsetAsync(kept_out, 0, 2 * sizeof(long long), s));
        return NEO_OK;
    }
    const int N0 = f.N0, N1 = f.N1;
    const neo::TpScene& sc = f.sc;
    const neo::TpViews& views = f.views;
    const size_t r = static_cast<size_t>(R);

    // workspaces: the dense layout (W[0..8]); W[9] holds the per-ray foreground results of BOTH levels (they are merged only after
    // the background has run) and the compact background results, W[10] the compaction's map / slot / count; a march adds the
    // point rows of one segment launch in W[12] and the per-row march state in W[13]
    auto* W = ctx->ws;
    int win_of[2] = {0, 0}, win_skip = 0;
    const neo::OccGrid* grid = nullptr;
    MarchState st{}, ot{};      // inside by ray; outside by compact row: the same bytes, read only after the inside marches are done
    if (o.stop_inside) {
        REQUIRE(r * N1 <= 2147483647UL, "too many points for 32-bit indices");
        const int skip_window = ctx->skip_window > 0 ? ctx->skip_window : SKIP_WINDOW_DEFAULT;
        win_of[0] = static_cast<int>(std::min<size_t>(r, std::max<size_t>(1, static_cast<size_t>(skip_window) * N0 / segment)));
        win_of[1] = static_cast<int>(std::min<size_t>(r, std::max<size_t>(1, static_cast<size_t>(skip_window) * N1 / segment)));
        const int win_max = std::max(win_of[0], win_of[1]);
        if (use_occ) grid = ctx->occ.get();
        // the rows of one launch: a segment of a window - or, with a grid and without `coarse`, all N0 samples of a window of
        // skip_window rays, the skipping frame's level 0, which follows no rule
        win_skip = grid && !coarse ? std::min(skip_window, R) : 0;
        const size_t launch_rows = std::max(static_cast<size_t>(win_max) * std::min(segment, N1), static_cast<size_t>(win_skip) * N0);
        REQUIRE(launch_rows * 3 <= 2147483647UL, "skip window too large for 32-bit indices");
        const size_t candidates = grid ? launch_rows : 0;      // with a grid: one keep byte per candidate behind the march state
        if (grid || (use_occ && ((samples0 && samples0->fg_keep) || (samples1 && samples1->fg_keep))))
            REQUIRE(r * N1 <= 2147483647UL - 1024, "too many points for 32-bit indices");
        if (W[13].reserve(std::max(MarchState::bytes(false, r, win_max, candidates), MarchState::bytes(true, r, win_max))))
            return NEO_ERR_NOMEM;
        st.carve(W[13].p, false, r, win_max);
        ot.carve(W[13].p, true, r, win_max);
    }
    TpDenseRows rows;
    if (rows.reserve(W, r, N0, N1) || W[9].reserve(r * 24 * 4) || W[10].reserve(neo::cull_ws_ints(R) * sizeof(int))) return NEO_ERR_NOMEM;
    // bg_s0 is the same row for every ray (k_tp_level0): its first `count` rows ARE the compact level-0 rows; bg_out, bg_w0 and
    // bg_s1 are compact: row k belongs to ray map[k]
    auto [far, fg_t0, bg_s0, fg_out, bg_out, fg_w0, bg_w0, fg_t1, bg_s1] = rows;
    float* scratch = W[9].as<float>();    // per level: fg_rgb(3) fg_depth fg_acc lambda bg_rgb(3) = 9 floats a ray; then compact bg_rgb(3) bg_depth, reused
    float* c_bg_rgb = scratch + r * 18;
    float* c_bg_depth = scratch + r * 21;
    int* cws = W[10].as<int>();
    const int* map = neo::cull_map_of(cws, R);
    const int* slot = neo::cull_slot_of(cws, R);
    const int* count = neo::cull_count_of(cws, R);

    neo::launch_sphere(rays_o, rays_d, R, far, nullptr, ctx->flags, s);       // sphere-miss assertions: every ray, stopped, culled or not
    neo::launch_tp_level0(far, f.edges, R, N0, f.near, fg_t0, bg_s0, s);
    const bool sigma0 = level0_sigma_only(level0);     // as neo_tp_render: density-only level-0 launches, no level-0 colour / depth
    const neo_tp_level_out* los[2] = {level0, level1};
    const neo_tp_march_samples* sos[2] = {samples0, samples1};
    struct LevelFg { float* fg_rgb; float* fg_depth; float* fg_acc; float* lam; float* bg_rgb; } L[2];
    for (int level = 0; level < 2; ++level) {
        const neo_tp_level_out* lo = los[level];
        float* b = scratch + r * 9 * level;
        L[level] = {(lo && lo->fg_rgb) ? lo->fg_rgb : b, b + r * 3, (lo && lo->fg_acc) ? lo->fg_acc : b + r * 4,
                    (lo && lo->bg_lambda) ? lo->bg_lambda : b + r * 5, lo ? lo->bg_rgb : nullptr};
    }
    // foreground of both levels first
    for (int level = 0; level < 2; ++level) {
        const int N = level == 0 ? N0 : N1;
        const float* fg_t = level == 0 ? fg_t0 : fg_t1;
        const neo_tp_march_samples* so = sos[level];
        const bool dens = level == 0 && sigma0;
        uint8_t* fg_keep = use_occ && so ? so->fg_keep : nullptr;       // the KEEP RULE on the whole row, behind the stops as well
        if (o.stop_inside && (level == 1 || coarse)) {
            if (int rc = tp_eval_march(ctx, f, a, MarchRule{true, eps, segment, 1, rays_d, far, nullptr, nullptr}, level, fg_t, N, fg_out,
                                       nullptr, st, win_of[level], kept ? kept + level : nullptr, false, grid))
                return rc;
        } else if (grid) {      // the grid alone: neo_tp_render_skipping's level 0, its mask straight into the caller's
            MarchState sk = st;
            if (fg_keep) sk.keep = fg_keep, sk.keep_dense = true;
            if (int rc = tp_eval_march(ctx, f, a, MarchRule{false, 0.0f, 0, 1, rays_d, far, nullptr, nullptr}, 0, fg_t, N, fg_out, nullptr, sk,
                                       win_skip, kept, false, grid))
                return rc;
            fg_keep = nullptr;
        } else {
            if (int rc = tp_launch(ctx, ctx->tp[level], sc, views, rays_o, rays_d, viewdirs, fg_t, nullptr, R, N, chunk, fg_out, s, nullptr, nullptr, dens)) return rc;
            if (o.stop_inside) neo::launch_march_init(nullptr, nullptr, nullptr, R, nullptr, nullptr, nullptr, st.stop, N, kept, N, s);
        }
        float* fg_w = level == 0 ? fg_w0 : (so ? so->fg_w : nullptr);
        neo::launch_composite(1, fg_out, fg_t, N, rays_d, far, R, N, 0, dens ? nullptr : L[level].fg_rgb, L[level].fg_acc,
                              dens ? nullptr : L[level].fg_depth, fg_w, L[level].lam, s);
        if (so) {
            const size_t row = r * N * sizeof(float);
            if (so->fg_t) HIP_TRY(hipMemcpyAsync(so->fg_t, fg_t, row, hipMemcpyDeviceToDevice, s));
            if (so->fg_w && level == 0) HIP_TRY(hipMemcpyAsync(so->fg_w, fg_w0, row, hipMemcpyDeviceToDevice, s));
            if (so->stop) HIP_TRY(hipMemcpyAsync(so->stop, st.stop, r * sizeof(int), hipMemcpyDeviceToDevice, s));
            if (so->fg_rows) HIP_TRY(hipMemcpyAsync(so->fg_rows, fg_out, row * 4, hipMemcpyDeviceToDevice, s));
            if (fg_keep)
                neo::launch_point_keep(neo::point_source_dense(rays_o, rays_d, fg_t, N, R, N), grid ? *grid : neo::OccGrid{},
                                       fg_keep, nullptr, s);
        }
        if (level == 0 && neo::launch_resample(fg_t0, N0, fg_w0, f.u, 0, R, N0, n_fine, 0, fg_t1, s))
            return fail(NEO_ERR_INVALID, "unsupported sample counts");
    }

    neo::launch_cull_compact(L[0].lam, L[1].lam, R, eps, cws, survivors_out, s);

    // One level's outside-sphere rows into the compact bg_out.  A level that follows the OUTSIDE STOP RULE marches (tp_eval_march);
    // any other is the culled frame's compact launch, and only a caller of the outside outputs pays for more: the counter, and
    // the rule's own kernel run to the end of the row (eps = 0 stops nothing) for stop = N and the running value there.
    auto background = [&](int level, const float* bg_s, int N, bool dens) -> int {
        const neo_tp_march_samples* so = sos[level];
        long long* kept_l = kept_out ? kept_out + level : nullptr;
        if (outside && (level == 1 || coarse)) {
            if (int rc = tp_eval_march(ctx, f, a, MarchRule{true, eps, segment, 2, rays_d, rows.far, L[level].lam, count}, level, bg_s, N,
                                       rows.bg_out, map, ot, win_of[level], kept_l, dens, nullptr))
                return rc;
        } else {
            if (int rc = tp_launch(ctx, ctx->tp[2 + level], sc, views, rays_o, rays_d, viewdirs, bg_s, rows.far, R, N, chunk, rows.bg_out, s, map,
                                   count, dens))
                return rc;
            const bool value = so && so->bg_value;
            if (kept_l || value || (so && so->bg_stop))
                neo::launch_march_init(L[level].lam, map, count, R, value ? ot.lam_c : nullptr, nullptr, value ? ot.value : nullptr, ot.stop,
                                       N, kept_l, N, s);
            if (value)
                neo::launch_march_advance(2, rows.bg_out, bg_s, N, nullptr, nullptr, ot.lam_c, N, 0, N, segment, 0.0f, nullptr, count, R, 0,
                                          nullptr, ot.value, nullptr, ot.stop, s);
        }
        if (so) {
            neo::launch_march_by_slot(ot.stop, ot.value, slot, R, so->bg_stop, so->bg_value, s);
            if (so->bg_rows) neo::launch_march_rows_by_slot(rows.bg_out, slot, R, N * 4, so->bg_rows, s);
        }
        return NEO_OK;
    };

    // background on the survivors
    if (int rc = background(0, bg_s0, N0, sigma0)) return rc;
    neo::launch_composite(2, bg_out, bg_s0, N0, nullptr, nullptr, R, N0, 0, sigma0 ? nullptr : c_bg_rgb, nullptr,
                          sigma0 ? nullptr : c_bg_depth, bg_w0, nullptr, s, count);
    if (neo::launch_resample(bg_s0, N0, bg_w0, f.u, 0, R, N0, n_fine, 1, bg_s1, s, count)) return fail(NEO_ERR_INVALID, "unsupported sample counts");
    if (level0 && (level0->rgb || level0->depth || level0->bg_rgb))
        neo::launch_tp_merge_culled(L[0].fg_rgb, L[0].fg_depth, L[0].lam, c_bg_rgb, c_bg_depth, slot, R, level0->rgb, level0->depth,
                                    L[0].bg_rgb, s);
    if (int rc = background(1, bg_s1, N1, false)) return rc;
    neo::launch_composite(2, bg_out, bg_s1, N1, nullptr, nullptr, R, N1, 0, c_bg_rgb, nullptr, c_bg_depth, nullptr, nullptr, s, count);
    if (level1 && (level1->rgb || level1->depth || level1->bg_rgb))
        neo::launch_tp_merge_culled(L[1].fg_rgb, L[1].fg_depth, L[1].lam, c_bg_rgb, c_bg_depth, slot, R, level1->rgb, level1->depth,
                                    L[1].bg_rgb, s);
    // bg_s: level 0 is one row for every ray (k_tp_level0); level 1 exists for the survivors only: a culled ray's row is zero
    if (samples0 && samples0->bg_s) HIP_TRY(hipMemcpyAsync(samples0->bg_s, bg_s0, r * N0 * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (samples1 && samples1->bg_s) neo::launch_march_rows_by_slot(bg_s1, slot, R, N1, samples1->bg_s, s);
    return check_launch();
}

// the dense foreground of both levels, the background on the rays whose bg_lambda is not below eps at both: the driver with nothing
// stopped
int neo_tp_render_culled(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                         const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse, int n_fine,
                         int white_bkgd, const neo_tp_level_out* level0, const neo_tp_level_out* level1, float eps,
                         int* survivors_out, void* stream) {
    ENTER(ctx);
    (void)white_bkgd;  // as neo_tp_render
    return tp_render_marching(ctx, {rays_o, rays_d, viewdirs, R, chunk, src_poses, NV, focal, cx, cy, n_coarse, n_fine, stream}, level0,
                              level1, eps, 0, 0, nullptr, nullptr, nullptr, nullptr, survivors_out,
                              {eps > 0.0f && eps < 1.0f ? nullptr : "eps must lie in (0, 1)", false, false, false});
}

int neo_tp_render_terminating(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                              const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse, int n_fine,
                              const neo_tp_level_out* level0, const neo_tp_level_out* level1, float eps, int segment, int coarse,
                              const neo_tp_term_samples* samples0, const neo_tp_term_samples* samples1, long long* kept,
                              int* survivors_out, void* stream) {
    ENTER(ctx);
    const neo_tp_term_samples* given[2] = {samples0, samples1};
    neo_tp_march_samples so[2];
    for (int l = 0; l < 2; ++l)
        if (given[l])
            so[l] = {given[l]->fg_t, given[l]->fg_w, given[l]->bg_s, given[l]->stop, nullptr, given[l]->fg_rows, nullptr, nullptr, nullptr};
    return tp_render_marching(ctx, {rays_o, rays_d, viewdirs, R, chunk, src_poses, NV, focal, cx, cy, n_coarse, n_fine, stream}, level0,
                              level1, eps, segment, coarse, samples0 ? &so[0] : nullptr, samples1 ? &so[1] : nullptr, kept, nullptr,
                              survivors_out, {march_arg_check(eps, segment), true, false, false});
}

// Occupancy skipping and early termination together (include/neo360_hip.h: ACCELERATED FRAME): the driver above with the grid read.
int neo_tp_render_accelerated(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                              const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse, int n_fine,
                              const neo_tp_level_out* level0, const neo_tp_level_out* level1, float eps, int segment, int coarse,
                              const neo_tp_accel_samples* samples0, const neo_tp_accel_samples* samples1, long long* kept,
                              int* survivors_out, void* stream) {
    ENTER(ctx);
    const neo_tp_accel_samples* given[2] = {samples0, samples1};
    neo_tp_march_samples so[2];
    for (int l = 0; l < 2; ++l)
        if (given[l])
            so[l] = {given[l]->fg_t, given[l]->fg_w, given[l]->bg_s, given[l]->stop, given[l]->fg_keep, given[l]->fg_rows, nullptr, nullptr,
                     nullptr};
    return tp_render_marching(ctx, {rays_o, rays_d, viewdirs, R, chunk, src_poses, NV, focal, cx, cy, n_coarse, n_fine, stream}, level0,
                              level1, eps, segment, coarse, samples0 ? &so[0] : nullptr, samples1 ? &so[1] : nullptr, kept, nullptr,
                              survivors_out, {march_arg_check(eps, segment), true, true, false});
}

// The driver itself (include/neo360_hip.h: MARCHING FRAME): use_grid chooses between the two calls above, `outside` adds the OUTSIDE
// STOP RULE; kept is int64[4], inside then outside per level.
int neo_tp_render_marching(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                           const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse, int n_fine,
                           const neo_tp_level_out* level0, const neo_tp_level_out* level1, float eps, int segment, int coarse,
                           int use_grid, int outside, const neo_tp_march_samples* samples0, const neo_tp_march_samples* samples1,
                           long long* kept, int* survivors_out, void* stream) {
    ENTER(ctx);
    return tp_render_marching(ctx, {rays_o, rays_d, viewdirs, R, chunk, src_poses, NV, focal, cx, cy, n_coarse, n_fine, stream}, level0,
                              level1, eps, segment, coarse, samples0, samples1, kept, kept ? kept + 2 : nullptr, survivors_out,
                              {march_arg_check(eps, segment), true, use_grid != 0, outside != 0});
}

// Object-level render: the two inside-sphere MLPs between a caller-given per-ray interval, on the rays that have one.
// Hit rule (objects.hip): lo = max(near_obj, 1e-4), hi = far_obj; hit iff both are finite and hi > lo, written as the negation of
// the failing comparisons (a NaN bound is a miss; the reference's 0 = "no hit" sentinel is one).
int neo_tp_render_objects(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, const float* near_obj,
                          const float* far_obj, int R, int chunk, const float* src_poses, int NV, float focal, float cx, float cy,
                          int n_coarse, int n_fine, int white_bkgd, const neo_tp_object_out* level0,
                          const neo_tp_object_out* level1, int* hits_out, void* stream) {
    ENTER(ctx);
    const TpFrameArgs a{rays_o, rays_d, viewdirs, R, chunk, src_poses, NV, focal, cx, cy, n_coarse, n_fine, stream};
    TpFrame::Own own;
    own.ptrs = near_obj && far_obj;
    TpFrame f;      // no outside-sphere slots, no ray-grid hint: every launch is compact
    if (int rc = f.begin(ctx, a, false, false, own)) return rc;
    hipStream_t s = f.s;
    if (f.empty) {
        if (hits_out) HIP_TRY(hipMemsetAsync(hits_out, 0, sizeof(int), s));
        return NEO_OK;
    }

    // workspaces: this lane's set.  Everything but the map is COMPACT (row k belongs to ray map[k]) and sized for R rows.
    auto* W = ctx->ws;
    TpCompactRows c;
    if (c.reserve(W, static_cast<size_t>(R), f.N0, f.N1) || W[10].reserve(neo::cull_ws_ints(R) * sizeof(int))) return NEO_ERR_NOMEM;
    int* cws = W[10].as<int>();
    const int* map = neo::cull_map_of(cws, R);
    const int* slot = neo::cull_slot_of(cws, R);
    const int* count = neo::cull_count_of(cws, R);

    neo::launch_obj_compact(near_obj, far_obj, R, cws, hits_out, s);
    neo::launch_obj_level0(near_obj, far_obj, rays_d, f.edges, map, count, R, f.N0, c.t0, c.far, c.rays_d, s);
    if (int rc = tp_march_compact(f, a, c, map, count, white_bkgd ? 1 : 0)) return rc;
    if (level0)
        neo::launch_obj_scatter(slot, R, f.N0, c.rgb[0], c.acc[0], c.depth[0], c.t0, white_bkgd, level0->rgb, level0->acc, level0->depth,
                                level0->tvals, s);
    if (level1)
        neo::launch_obj_scatter(slot, R, f.N1, c.rgb[1], c.acc[1], c.depth[1], c.t1, white_bkgd, level1->rgb, level1->acc, level1->depth,
                                level1->tvals, s);
    return check_launch();
}

}  // extern "C"
