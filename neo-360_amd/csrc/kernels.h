// Host-side launch wrappers implemented by the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace neo {

// rays.hip
// rays [ray0, ray0 + n) of the H x W frame -> rows [0, n) of the outputs
void launch_raygen(int H, int W, float focal, const float* c2w, int ray0, int n, float* rays_o, float* viewdirs,
                   float* rays_d, float* radii, hipStream_t s);
struct BoxFrame {        // one oriented box: world -> box frame (row-major 3x4 of a 4x4, float64) and its bounds
    double m[12];
    double lo[3], hi[3];
};
void launch_aabb_multi(const BoxFrame* boxes_dev, int n_boxes, const double* rays_o, const double* rays_d, int R,
                       uint8_t* hit_per_box, float* near, float* far, uint8_t* mask, hipStream_t s);
// the same transform and slab test, every box's own interval: near / far (n_boxes, R) float32 with 0 = no hit, hit (n_boxes, R)
void launch_aabb_per_box(const BoxFrame* boxes_dev, int n_boxes, const double* rays_o, const double* rays_d, int R, float* near,
                         float* far, uint8_t* hit, hipStream_t s);
void launch_aabb(const double* bounds, const double* rays_o, const double* rays_d, int R, uint8_t* hit,
                 double* tmin, double* tmax, hipStream_t s);
void launch_sphere(const float* rays_o, const float* rays_d, int R, float* far, uint8_t* ok, uint32_t* flags,
                   hipStream_t s);

// sampling.hip
void launch_pos_enc(const float* x, int n, int C, int min_deg, int max_deg, float* out, hipStream_t s);
// r_dev (composite, resample): null, or a device word holding the number of rows actually present (<= R): the grid is sized for R
// and the surplus leaves early - compact arrays whose length the host never reads (cull.hip)
// mode 0 vanilla, 1 NeO-360 inside sphere, 2 NeO-360 outside sphere.
void launch_composite(int mode, const float* rgbsigma, const float* t, int t_row_stride, const float* rays_d,
                      const float* t_far, int R, int N, int white_bkgd, float* rgb, float* acc, float* depth, float* weights,
                      float* lambda, hipStream_t s, const int* r_dev = nullptr);
// u: n_new quantiles (device), see Ctx::quantiles; u_row_stride 0 = one row shared by all rays (randomized=False),
// n_new = one row per ray (randomized=True: uniform draws)
int launch_resample(const float* t_prev, int t_prev_stride, const float* weights, const float* u, int u_row_stride, int R,
                    int n_prev, int n_new, int descending, float* t_out, hipStream_t s, const int* r_dev = nullptr);

// training.hip — training-side operators
void launch_uniform(uint64_t seed, uint32_t stream, int rows, int cols, float* out, hipStream_t s);
// dst[b][c][r] = src[b][r][c] (batched 2-D transpose, tiled through LDS)
void launch_transpose(const float* src, long batch, int rows, int cols, float* dst, hipStream_t s);
void launch_tp_level0_rand(const float* far, const float* edges, int R, int N, float near, const float* u_fg,
                           const float* u_bg, float* fg_t, float* bg_s, hipStream_t s);
int launch_composite_bwd(int mode, const float* rgbsigma, const float* t, int t_row_stride, const float* rays_d,
                         const float* t_far, int R, int N, int white_bkgd, const float* g_rgb, const float* g_acc,
                         const float* g_depth, const float* g_w, const float* g_lam, float* g_rgbsigma, hipStream_t s);
void launch_distloss(const float* w, const float* m, int R, int N, float interval, float* loss_rays, float* grad_w,
                     hipStream_t s);
struct TpScene;
struct TpViews;
void launch_gather(const TpScene& sc, const TpViews& views, const float* pts, long P, float* world, float* local,
                   hipStream_t s);
// lookup in a caller-owned channels-last map (NV Hf Wf, C) at the latent's taps (C % 64 == 0) and its run-merged scatter backward;
// pitch > 0: the map's row pitch in floats (a C-column slice of a wider map: `map` / `g_map` point at the slice's first column)
void launch_map_gather(const TpScene& sc, const TpViews& views, const float* pts, long P, const float* map, int C, float* out,
                       hipStream_t s, long pitch = 0);
void launch_map_gather_bwd(const TpScene& sc, const TpViews& views, const float* pts, long P, const float* g_out, int C, float* g_map,
                           hipStream_t s, long pitch = 0);
// training call: lookup points (P,3) + per-view reference-order encodings (NV,P,21 C) of the samples tvals (R,N); input_ch 3 inside /
// 4 outside the sphere (far required); activations (raw -> (rgb, sigma) packed) with their backward
void launch_tp_train_points(int input_ch, const float* rays_o, const float* rays_d, const float* tvals, const float* far, int R, int N,
                            const TpViews& views, int nv, uint32_t* flags, float* look, float* x_enc, hipStream_t s);
void launch_tp_activate(const float* raw_rgb, const float* raw_sigma, const float* noise, float noise_scale, long P, float* rgbsigma,
                        hipStream_t s);
void launch_tp_activate_bwd(const float* raw_rgb, const float* raw_sigma, const float* noise, float noise_scale, long P,
                            const float* g_rgbsigma, float* g_rgb, float* g_sigma, hipStream_t s);
void launch_gather_bwd(const TpScene& sc, const TpViews& views, const float* pts, long P, const float* g_world,
                       const float* g_local, float* g_plane_xz, float* g_plane_xy, float* g_plane_yz, float* g_latent,
                       hipStream_t s);

// mlp_vanilla.hip
struct VanillaMlpDev {
    const float* wpack;   // packed GEMM stages (fragment order)
    const float* bias;    // concatenated per-stage biases
    const float* heads;   // density w[256], density b, rgb w[3][128], rgb b[3]
};
size_t vanilla_wpack_floats();
size_t vanilla_bias_floats();
size_t vanilla_heads_floats();
void launch_vanilla_pack(const float* const* weights, const float* const* biases, float* wpack, float* bias,
                         float* heads, hipStream_t s);
// mlp_vanilla_h.hip — the same MLP on the fp16 matrix cores with hi/lo-split operands (fp32-equivalent)
struct VanillaMlpHDev {
    const void* wpack;    // fp16 hi/lo fragments
    const float* bias;    // shared with the fp32 path
    const float* heads;
    uint32_t* flags;      // context assertion word (bit 1: split range guard)
};
size_t vanilla_wpack_h_bytes();
// pack_h.hip: [W_v[:, :nb] . W_b | W_v[:, nb:]] and b_v + W_v[:, :nb] . b_b - a linear bottleneck folded into the layer that consumes it
void launch_fold_bottleneck(const float* wv, const float* wb, const float* bb, const float* bv, int n_out, int nb, int nin,
                            int extra, float* wfold, float* bfold, hipStream_t s);
// biases / fold_ws: the split kernel folds the (linear) bottleneck into the view layer at pack time: bias_h = its own copy of the
// bias block with the view layer's entry replaced, fold_ws = vanilla_fold_floats() floats of scratch
size_t vanilla_fold_floats();
void launch_vanilla_pack_h(const float* const* weights, const float* const* biases, void* wpack_h, float* fold_ws,
                           const float* bias_src, float* bias_h, hipStream_t s);
void launch_vanilla_mlp_h(const VanillaMlpHDev& m, const float* rays_o, const float* dirs, const float* t,
                          int t_row_stride, int R, int N, float* out, hipStream_t s);
void launch_vanilla_mlp(const VanillaMlpDev& m, const float* rays_o, const float* dirs, const float* t,
                        int t_row_stride, int R, int N, float* out, hipStream_t s);
// The compact launches of the two evaluators (vanilla_march.hip): rays_o, dirs (cap,3), t (cap), out (cap,4), all allocated for
// `cap` rows, the host's bound, of which min(*count, cap) are live (count: a device word; 0 is a valid launch).  Row k is ONE point,
// rays_o[k] + t[k] dirs[k] seen along dirs[k]; its out row is bitwise the dense launch's for the same point.  Rows behind the count
// are neither read nor written, and the variant (waves, tile) follows the process's setting, never the count.
void launch_vanilla_mlp_h_compact(const VanillaMlpHDev& m, const float* rays_o, const float* dirs, const float* t, long cap,
                                  const int* count, float* out, hipStream_t s);
void launch_vanilla_mlp_compact(const VanillaMlpDev& m, const float* rays_o, const float* dirs, const float* t, long cap,
                                const int* count, float* out, hipStream_t s);

// mlp_tp.hip — NeO-360 decoder
constexpr int TP_MAX_VIEWS = 8;
struct TpMlpDev {
    const float* wpack;
    const float* bias;
    const float* heads;
};
struct TpScene {                     // channels-last feature maps owned by the context
    const float* latent;            // (NV, Hf, Wf, 512)
    const float* plane[3];          // xz, xy, yz: (NV, Hp, Wp, 128)
    int nv, Hf, Wf, Hp, Wp;
    float focal, cx, cy;            // source view 0's intrinsics (neo360/model.py:242-244)
    float sx, sy;                   // latent_scaling / image_size (encoder_pn.py:121-123, :204-206)
    float fy_sign = -1.0f;          // v = (-y/z) * (fy_sign * focal) + cy: -1 for NeRF_TP (model.py:243), +1 for the
                                    // PixelNeRF baseline, which passes (f, f) (vanilla_nerf/model_pixel.py:203-206)
    // Ray-patch tile order (round 6, neo_ctx_set_ray_grid): when the rays of a launch are pixels of a row-major image of width
    // grid_w (ray 0 of the launch = pixel grid_first of the frame), the evaluators walk the rays of every whole band of 2^grid_ph
    // image rows in 2^grid_pw x 2^grid_ph pixel PATCHES instead of row by row, so the ~64 tiles resident on an XCD cover a compact
    // piece of the image and share feature texels in that XCD's L2 in both image directions (shape chosen per region in
    // api_tp.hip:tp_launch).  0: rays in the caller's order.  Results do not depend on it.
    int grid_w = 0;
    long grid_first = 0;
    int grid_pw = 3, grid_ph = 3;   // log2 of the patch width / height in pixels (bands are 2^grid_ph image rows)
    // Quad order (point_order.h:quad_point; policy in api_tp.hip:tp_launch): the pre-projected split evaluators interleave the
    // samples of `quad` consecutive launch-order rays (4 = a quad, 8, 16: a multiple of 4), so that the four rows of one gather
    // instruction are four neighbouring rays at one sample index.  0 (default): ray-major.  Compact launches never use it.
    // Results do not depend on it.
    int quad = 0;
    // Compact launch (neo_tp_render_culled, cull.hip; neo_tp_render_objects, objects.hip): row g' of the launch stands for sample g' % N of ray cull_map[g' / N];
    // tvals and the output are indexed by g', the rays' own arrays and the quirk-Q1 direction index by the ray and the
    // launch's R.  The launch holds *cull_count rays (device word, never read on the host): the grid is sized for R and the
    // surplus workgroups exit.  Null (every other caller): rows are the caller's rays.  grid_w must be 0 with a map.
    const int* cull_map = nullptr;
    const int* cull_count = nullptr;
};
struct TpViews {                     // world -> camera per source view (neo360/util.py:52-70)
    float rot[TP_MAX_VIEWS][9];     // c2w[:3,:3]^T, row-major
    float trans[TP_MAX_VIEWS][3];   // -rot @ c2w[:3,3]
};
size_t tp_wpack_floats(int input_ch);
size_t tp_bias_floats();
size_t tp_heads_floats();
// fold_ws: tp_fold_floats() floats of scratch (stage V0F: view layer 0 with the bottleneck folded in)
void launch_tp_pack(int input_ch, const float* const* w, const float* const* b, float* wpack, float* bias,
                    float* heads, hipStream_t s, float* fold_ws);
void launch_channels_last(const float* src, int NV, int C, int H, int W, float* dst, hipStream_t s);
struct TpPlaneProj;
// proj != null: the latent pre-projected through [W0_loc | W3_loc] is gathered instead of the latent (k_tp_preproject);
// pp != null as well: the three tri-planes pre-projected through [W0_world | W3_world] likewise.  With proj the kernel reads the
// view-summed direction encodings from `dirsum` (rays, 32; launch_tp_dirsum below, on the same stream before this launch)
void launch_tp_mlp(int input_ch, const TpMlpDev& m, const TpScene& sc, const TpViews& views, const float* rays_o,
                   const float* rays_d, const float* viewdirs, const float* tvals, const float* far, int R, int N,
                   int chunk, uint32_t* flags, float* out, hipStream_t s, const float* proj = nullptr,
                   const TpPlaneProj* pp = nullptr, const float* dirsum = nullptr);

// weight re-packing into MFMA fragment order (defined in mlp_tp.hip)
struct PackSegs { int k0[3], len[3], col[3]; };
struct PackPerm { short col[256]; };      // packed k -> source column (-1: zero), passed by value (pack_h_perm)
void pack_block(const float* src, int ld, int rows, int KC, int nt0, PackSegs sg, float* dst, hipStream_t s);
void copy_floats(const float* src, int n, float* dst, hipStream_t s);

// mlp_mip.hip / mip_sampling.hip — Mip-NeRF 360
struct MipMlpDev {
    const float* wpack;
    const float* bias;
    const float* heads;
    const float* basis;   // (3,21) row-major
};
struct MipMlpHDev {       // split-fp16 fragments (mlp_mip_h.hip); bias / heads / basis shared with MipMlpDev
    const void* wpack;
    const float* bias;
    const float* heads;
    const float* basis;
    uint32_t* flags;      // context assertion word (bit 1: split range guard)
    const float* view_bias = nullptr;   // 128: views_linear.0's bias with the bottleneck folded in (b_v + W_v[:, :256] b_b); rgb MLP only
};
size_t mip_wpack_h_bytes(int width, int depth, int rgb);
size_t mip_fold_floats();     // scratch of launch_mip_pack_h (the folded view layer, fp32)
// rgb MLP: the (linear) bottleneck is folded into views_linear.0 at pack time (pack_h.hip:launch_fold_bottleneck): the fragments
// hold [W_v[:, :256] W_b | W_v[:, 256:]] (128 x (width + 27)), view_bias (128 floats) receives the folded bias
void launch_mip_pack_h(int width, int depth, int rgb, const float* const* w, const float* const* b, void* wpack_h, float* fold_ws,
                       float* view_bias, hipStream_t s);
int launch_mip_mlp_h(int width, int depth, int rgb, const MipMlpHDev& m, const float* rays_o, const float* rays_d,
                     const float* viewdirs, const float* radii, const float* tdist, int R, int n, float* out,
                     hipStream_t s);
size_t mip_wpack_floats(int width, int depth, int rgb);
size_t mip_bias_floats(int width, int depth, int rgb);
size_t mip_heads_floats(int width);
// w/b order: pts_linear.0..depth-1, density_layer[, bottleneck_layer, views_linear.0, rgb_layer]
void launch_mip_pack(int width, int depth, int rgb, const float* const* w, const float* const* b, float* wpack,
                     float* bias, float* heads, hipStream_t s);
int launch_mip_mlp(int width, int depth, int rgb, const MipMlpDev& m, const float* rays_o, const float* rays_d,
                   const float* viewdirs, const float* radii, const float* tdist, int R, int n, float* out,
                   hipStream_t s);
// one wave per ray: (optional max-dilate of the previous histogram) -> annealed logits -> softmax cdf ->
// n centre quantiles (u, device table) -> interval endpoints sdist (R,n+1) and metric distances tdist
int launch_mip_resample(const float* s_prev, const float* w_prev, int n_prev, int dilate, float dilation,
                        float anneal, const float* u, int R, int n, float s_near, float s_far, float* sdist,
                        float* tdist, hipStream_t s, const float* jitter = nullptr);
// weights = alpha * exp(-cumsum) with an opaque last interval; rgb = sum w c + max(0,1-acc) * bg
void launch_mip_composite(const float* rgbdens, const float* tdist, const float* rays_d, int R, int n, float bg,
                          float* weights, float* rgb, hipStream_t s);

// mip_losses.hip — Mip-NeRF 360's interlevel and distortion losses (helper.py:108-148), one wave per ray, fp64 between fp32 ends.
// t (R,N+1) / w (R,N): the histogram whose loss is taken; t_env (R,Ne+1) / w_env (R,Ne): a proposal level's; edges non-decreasing.
// loss (R,N); backward: g_loss (R,N) -> g_w (R,N), g_w_env (R,Ne), either may be null.  Return -1 outside 1 <= N, Ne <= 1024.
int launch_mip_lossfun_outer(const float* t, const float* w, const float* t_env, const float* w_env, int R, int N, int Ne, float* loss,
                             hipStream_t s);
int launch_mip_lossfun_outer_bwd(const float* t, const float* w, const float* t_env, const float* w_env, const float* g_loss, int R, int N,
                                 int Ne, float* g_w, float* g_w_env, hipStream_t s);
// loss_rays (R) and, when not null, d loss_ray / d w (R,N)
int launch_mip_lossfun_distortion(const float* t, const float* w, int R, int N, float* loss_rays, float* grad_w, hipStream_t s);

// mip_extras.hip — opacity, expected distance and distance percentiles of an interval histogram, one wave per ray, fp64 between fp32
// ends.  edges (R,n+1) non-decreasing: metric distances when near == far == 0, else sdist mapped with s_to_t; w (R,n); u (n_u) device
// quantiles -> acc (R), dist_mean (R), dist_pct (R,n_u), each may be null.  Backward: g_acc (R), g_mean (R), either may be null
// -> g_w (R,n).  Return -1 outside 1 <= n <= 1024, 0 <= n_u <= 8, or when exactly one of near / far is zero.
int launch_mip_extras(const float* edges, const float* w, int R, int n, float near, float far, const float* u, int n_u, float* acc,
                      float* dist_mean, float* dist_pct, hipStream_t s);
int launch_mip_extras_bwd(const float* edges, const float* w, int R, int n, float near, float far, const float* g_acc,
                          const float* g_mean, float* g_w, hipStream_t s);

// tp_extras.hip — opacity, expected disparity and distance percentiles of a NeO-360 ray's whole interval histogram (inside + outside
// the sphere) as distances along the ray, one wave per ray, fp64 between fp32 ends.  fg_t / fg_w (R,N), far (R): the inside rows and
// the sphere exit; bg_s / bg_w (R,N), lambda (R): the outside rows (inverse radius, descending) and the inside composite's last
// transmittance - all three null: the inside-only histogram; rays_o / rays_d (R,3); u (n_u) device quantiles -> opacity (R),
// disparity (R), dist_pct (R,n_u), each may be null.  Return -1 outside 1 <= N <= 1024, 0 <= n_u <= 8, or when only some of the
// three outside pointers are given.
int launch_tp_extras(const float* fg_t, const float* fg_w, const float* far, const float* bg_s, const float* bg_w, const float* lambda,
                     const float* rays_o, const float* rays_d, int R, int N, const float* u, int n_u, float* opacity, float* disparity,
                     float* dist_pct, hipStream_t s);

// mlp_tp_h.hip — the NeO-360 evaluator on the fp16 matrix cores (hi/lo-split operands, fp32-equivalent)
struct TpMlpHDev {
    const void* wpack;    // fp16 hi/lo fragments
    const float* bias;    // shared with the fp32 path
    const float* heads;
    uint32_t* flags;      // context assertion word (bit 0: unit-sphere miss, bit 1: split range guard)
};
// Range checks backing the split-fp16 guard (pack_h.hip): any fp16 inf / NaN among n packed halves (a weight
// >= 65520 in magnitude, or non-finite), any fp32 value with |x| >= limit or non-finite -> flags |= 2.
void launch_half_range_check(const void* halves, size_t n, uint32_t* flags, hipStream_t s);
void launch_f32_range_check(const float* x, size_t n, float limit, uint32_t* flags, hipStream_t s);
// The low end of the guard.  hi = fp16(w) keeps 11 bits and lo = fp16(w - hi) the next 11 only while lo is an fp16 normal; below
// |w| ~ 2^-3 the lo plane runs into the subnormals and below 2^-13 it holds nothing, so the error of a product stays at about
// 2^-25 per operand however small the operand: a layer whose weights are ALL small loses relative accuracy in proportion.
// Rule: a linear layer with 0 < max |w| < SPLIT_WEIGHT_LOW trips the guard as a static operand (an all-zero layer splits
// exactly).  2^-13 is taken from the measured error-against-scale curve of the dense evaluators (docs/dense_mlp_sweep.md).
// launch_abs_max folds max |x| over n floats into *out (bits of a non-negative float, zeroed by the caller);
// launch_weight_low_end_check reads nl such maxima and raises flag bits 1 and 2 when one of them is inside (0, low).
constexpr float SPLIT_WEIGHT_LOW = 0x1p-13f;
// The 128-wide decoder MLPs and the 512-wide pillar stage reach half of their per-entry bounds at larger weights than the dense
// 256 / 1024-wide evaluators; each value below is the smallest power of two that flags every state of tests/split_scale_cases.py
// measured above half a bound AND keeps the share extrapolated to the threshold itself (error ~ 1 / operand) at or under half, for
// every rescaling kind of the family (docs/split_scale_sweep.md has the curves; largest |w| of the last state at or under half /
// of the first one above it in brackets):
constexpr float SPLIT_WEIGHT_LOW_TP = 0x1p-11f;    // NeO-360 decoder slots (views_linear.0: 1.25e-3 at 0.13 / 3.1e-4 at 0.66)
constexpr float SPLIT_WEIGHT_LOW_PIX = 0x1p-9f;    // PixelNeRF slots (pts_linears.2: 2.4e-3 at 0.22 / 6.0e-4 at 0.87)
constexpr float SPLIT_WEIGHT_LOW_ENC = 0x1p-6f;    // pillar stage (depth_fc.common_branch.0: 1.9e-2 at 0.30 / 4.9e-3 at 0.96)
// The same rule for an fp32 feature map that a split kernel reads RAW (not through the fp32 pre-projection): a map whose largest
// |x| is inside (0, low) trips the guard - an uploaded scene map as a static operand, the pillar stage's latent per call.
constexpr float SPLIT_MAP_LOW = 0x1p-8f;           // tri-planes / latent of the decoders (2.3e-3 at 0.46 / 5.9e-4 at 1.9)
constexpr float SPLIT_LATENT_LOW_ENC = 0x1p-6f;    // pillar stage's latent (3.6e-2 at 0.15 / 9.0e-3 at 0.61)
void launch_abs_max(const float* x, size_t n, uint32_t* out, hipStream_t s);
// skip_mask: bit i set = maximum i is not looked at (a layer the launched fragment set folds into another one in fp64 at pack
// time); static_operand: raise bit 2 beside bit 1
void launch_low_end_check(const uint32_t* maxima, int n, float low, uint32_t skip_mask, bool static_operand, uint32_t* flags, hipStream_t s);
inline void launch_weight_low_end_check(const uint32_t* wmax, int nl, float low, uint32_t* flags, hipStream_t s) {
    launch_low_end_check(wmax, nl, low, 0u, true, flags, s);
}
size_t tp_wpack_h_bytes(int input_ch);
void launch_tp_pack_h(int input_ch, const float* const* w, void* wpack_h, hipStream_t s);
void launch_tp_mlp_h(int input_ch, const TpMlpHDev& m, const TpScene& sc, const TpViews& views, const float* rays_o,
                     const float* rays_d, const float* viewdirs, const float* tvals, const float* far, int R, int N,
                     int chunk, uint32_t* flags, float* out, hipStream_t s);

// mlp_tp_hp.hip — the split-fp16 evaluator on the latent pre-projected through [W0_loc | W3_loc] (default)
int tp_kc_x(int input_ch);            // k-chunks per N-tile of stage X in the fp32 fragment pack (mlp_tp.hip)
size_t tp_wpack_hp_bytes(int input_ch);
size_t tp_proj_bytes(long texels);    // pre-projected map: 256 fp32 channels per latent texel
// fold_ws: tp_fold_floats() floats of scratch (the folded view-layer-0 matrix, tp_hp_layout.h NEO_TP_FOLDB); bias_src: the shared
// 768-float bias block; bias_hp: the pre-projected evaluators' own copy of it (view layer 0's bias folded)
size_t tp_fold_floats();
void launch_tp_pack_hp(int input_ch, const float* const* w, const float* const* b, void* wpack_hp, float* fold_ws,
                       const float* bias_src, float* bias_hp, hipStream_t s);
// G (texels, 256) = latent_cl (texels, 512) . [W0_loc | W3_loc]^T from the fp32 fragment pack's stage X
// (in_ch = 128, first_chunk = 64: a tri-plane through the world columns [W0_world | W3_world], mlp_tp_hpp.hip)
void launch_tp_preproject(const float* latent_cl, long texels, const float* wpack_f32_stage_x, int kc_x, float* proj,
                          hipStream_t s, int channels = 256, int in_ch = 512, int first_chunk = 0);
// dirsum (R, 32): per ray the SUM over the source views of its view-direction encoding in each view's camera frame
// (27 features + 5 zeros), built by launch_tp_dirsum before every evaluator launch.
// density_only (both launchers below): the caller reads the launch's sigma only - the kernel may skip the colour branch (direction
// staging, view layers, rgb head), writes rgb = 0 and does not read `dirsum` (may be null).  A permission, not a contract: a launch
// without a density-only instantiation (the object render's compact one) computes everything.
void launch_tp_dirsum(const float* viewdirs, int R, const TpViews& views, int nv, float* dirsum, hipStream_t s);
void launch_tp_mlp_hp(int input_ch, const TpMlpHDev& m, const float* proj, const TpScene& sc, const TpViews& views,
                      const float* rays_o, const float* rays_d, const float* viewdirs, const float* tvals,
                      const float* far, int R, int N, int chunk, uint32_t* flags, float* out, const float* dirsum,
                      hipStream_t s, bool density_only = false);

// mlp_tp_hpp.hip — the same evaluator with the three TRI-PLANES pre-projected as well (through [W0_world | W3_world]):
// no world GEMM stage per point-view; 4 maps x 1 KB taps are blended and added to the L0 / L3-skip accumulators
struct TpPlaneProj { const float* p[3]; };      // xz, xy, yz: (NV * Hp * Wp, 256) fp32, channel order hp::proj_index
// proj_all: ONE buffer [projected latent | projected xz | xy | yz] (+ >= 4 KB of padding: the gather pipeline reads one
// chunk past its last item); plane_base_texels[j]: first texel (1 KB each) of plane j in it; total size < 4 GB.
size_t tp_proj_pad_bytes();
void launch_tp_mlp_hpp(int input_ch, const TpMlpHDev& m, const float* proj_all, const long plane_base_texels[3],
                       const TpScene& sc, const TpViews& views, const float* rays_o, const float* rays_d, const float* viewdirs,
                       const float* tvals, const float* far, int R, int N, int chunk, uint32_t* flags, float* out,
                       const float* dirsum, hipStream_t s, bool density_only = false);

// (train_mlp.hip's launchers are declared in train_kernels.h)

// mlp_pix_h.hip — PixelNeRF baseline decoder evaluator, split-fp16 arithmetic (the default)
size_t pix_wpack_h_bytes();
size_t pix_bias_floats();
size_t pix_heads_floats();
size_t pix_fold_floats();        // scratch of launch_pix_pack_h (the folded view-layer-0 matrix)
void launch_pix_pack_h(const float* const* w, const float* const* b, void* wpack_h, float* bias, float* heads,
                       float* fold_ws, hipStream_t s);
void launch_pix_mlp_h(const TpMlpHDev& m, const float* proj /* null: gather the latent itself */, const TpScene& sc, const TpViews& views, const float* rays_o,
                      const float* rays_d, const float* viewdirs, const float* tvals, int t_shared, int R, int N,
                      int chunk, float* out, hipStream_t s);

// mlp_pix.hip — the same decoder in EXACT fp32 MFMA arithmetic, latent gathered as the reference gathers it (round 5)
size_t pix_wpack_floats();
int pix_kc_x();                  // k-chunks per N-tile of its first stage (the first 64 = the latent columns k_tp_preproject reads)
void launch_pix_pack(const float* const* w, const float* const* b, float* fold_v0, const float* bias_src, float* bias_f32,
                     float* wpack, hipStream_t s);
void launch_pix_mlp(const TpMlpDev& m, const TpScene& sc, const TpViews& views, const float* rays_o, const float* rays_d,
                    const float* viewdirs, const float* tvals, int t_shared, int R, int N, int chunk, float* out, hipStream_t s);
// The compact launches of the two PixelNeRF evaluators (api_pix.hip), the contract of launch_vanilla_mlp_h_compact above with a
// view column: rays_o, rays_d, viewdirs (cap,3), t (cap), out (cap,4), all allocated for `cap` rows, the host's bound, of which
// min(*count, cap) are live (count: a device word; 0 is a valid launch).  Row k is ONE point, rays_o[k] + t[k] rays_d[k], seen
// along viewdirs[k] - the caller has already resolved quirk Q1, the launch treats every row as its own ray (N = 1, one chunk).
// Its out row is bitwise the dense launch's for the same point and direction, in both operation orders (proj or not) and both
// arithmetics.  Rows at or behind the count are neither read nor written; the variant never depends on the count.
void launch_pix_mlp_h_compact(const TpMlpHDev& m, const float* proj, const TpScene& sc, const TpViews& views, const float* rays_o,
                              const float* rays_d, const float* viewdirs, const float* t, long cap, const int* count, float* out,
                              hipStream_t s);
void launch_pix_mlp_compact(const TpMlpDev& m, const TpScene& sc, const TpViews& views, const float* rays_o, const float* rays_d,
                            const float* viewdirs, const float* t, long cap, const int* count, float* out, hipStream_t s);

// pillar.hip — pillar stage of the scene encoder
struct PillarGeom {
    int nv, G0, G1, G2;                // rows = nv * G0 * G1 * G2, x slowest (neo360/util.py:12-26)
    int Hf, Wf;
    float focal, cx, cy, sx, sy;       // view 0's intrinsics; latent_scaling / image size
    const float* axes;                 // device: torch.linspace values of the three axes, [3][256]
    float rot[TP_MAX_VIEWS][9], trans[TP_MAX_VIEWS][3], cpos[TP_MAX_VIEWS][3];
};
size_t pillar_wpack_bytes();
// w: depth_fc.common_branch.0 (512x518), .2, depth_fc.depth_encoder, pillar_aggregator_{xz,yz,xy}.0 (512x513)
void launch_pillar_pack(const float* const* w, void* wpack, hipStream_t s);
// bias: 6 x 512 in that order; head_w: pillar_aggregator_{xz,yz,xy}.2 weights (3 x 512); head_b_host: their biases;
// h1, h2, Lf: (M,512) workspaces, score (3,M); outputs channels-last floor-plans.  Returns -1 for unsupported grids.
int launch_pillar(const PillarGeom& gm, const float* latent_cl, const void* wpack, const float* bias, const float* head_w,
                  const float* head_b_host, float* h1, float* h2, float* Lf, float* score, uint32_t* flags, float* fp_yz,
                  float* fp_xz, float* fp_xy, hipStream_t s);

// sampling.hip — NeO-360 level-0 sample rows and fg/bg merge
void launch_tp_level0(const float* far, const float* edges, int R, int N, float near, float* fg_t, float* bg_s,
                      hipStream_t s);
void launch_tp_merge(const float* fg_rgb, const float* fg_depth, const float* lambda, const float* bg_rgb,
                     const float* bg_depth, int R, float* rgb, float* depth, hipStream_t s);

// cull.hip - background culling of neo_tp_render_culled: stable compaction of the rays whose foreground still lets light through
size_t cull_ws_ints(int R);        // ints of workspace for R rays: [map R | slot R | count 1 | block totals]
// keep[ray] = !(lam0 < eps) || !(lam1 < eps) (a NaN survives); map[k] = k-th kept ray (ascending), slot[ray] = k or -1, *count = kept
// rays (also written to *count_out when not null).  Two launches, no atomics: the same map on every run.
void launch_cull_compact(const float* lam0, const float* lam1, int R, float eps, int* ws, int* count_out, hipStream_t s);
inline int* cull_map_of(int* ws, int R) { (void)R; return ws; }
inline int* cull_slot_of(int* ws, int R) { return ws + R; }
inline int* cull_count_of(int* ws, int R) { return ws + 2 * (size_t)R; }
// merge of a culled render: survivors as launch_tp_merge from the COMPACT background rows bg_rgb_c / bg_depth_c at slot[ray];
// a culled ray gets rgb = fg_rgb, depth = fg_depth; bg_rgb (R,3, may be null) receives the survivor's background or exactly 0
void launch_tp_merge_culled(const float* fg_rgb, const float* fg_depth, const float* lambda, const float* bg_rgb_c,
                            const float* bg_depth_c, const int* slot, int R, float* rgb, float* depth, float* bg_rgb, hipStream_t s);

// objects.hip - object render of neo_tp_render_objects: the rays with a box interval, compacted as above (same workspace layout:
// cull_ws_ints / cull_map_of / cull_slot_of / cull_count_of)
// hit[ray] = near_obj, far_obj finite && far_obj > max(near_obj, 1e-4), written as the negation of the failing comparisons (a NaN
// bound is a miss); *count = hit rays (also written to *count_out when not null)
void launch_obj_compact(const float* near_obj, const float* far_obj, int R, int* ws, int* count_out, hipStream_t s);
// compact level-0 rows: t0_c (count, N) = lo (1 - e) + hi e, far_c (count) = hi, rays_d_c (count, 3); grid sized for R rows
void launch_obj_level0(const float* near_obj, const float* far_obj, const float* rays_d, const float* edges, const int* map,
                       const int* count, int R, int N, float* t0_c, float* far_c, float* rays_d_c, hipStream_t s);
// hit rays copy compact rgb / acc / depth (and the t rows, (count, N)) to their ray; missed rays get rgb = white_bkgd ? 1 : 0,
// acc = depth = 0 and a zero t row.  Any output may be null.
void launch_obj_scatter(const int* slot, int R, int N, const float* rgb_c, const float* acc_c, const float* depth_c,
                        const float* t_c, int white_bkgd, float* rgb, float* acc, float* depth, float* tvals, hipStream_t s);

// instances.hip - instance render of neo_tp_render_instances: the hit (instance, ray) PAIRS of K x R intervals, pair = i R + ray,
// compacted as above over K R elements (the hit rule of objects.hip per pair) and consumed in K windows of at most R rows
size_t inst_ws_ints(int K, int R);      // [cull_ws_ints(K R) | ray map of the current window R | window counts K]
inline int* inst_raymap_of(int* ws, int K, int R) { return ws + cull_ws_ints(K * R); }
inline int* inst_wcount_of(int* ws, int K, int R) { return inst_raymap_of(ws, K, R) + R; }
// pair map / count at cull_map_of / cull_count_of (ws, K R); wcount[p] = min(max(count - p R, 0), R); *count_out = count
void launch_inst_compact(const float* near_inst, const float* far_inst, int K, int R, int* ws, int* count_out, hipStream_t s);
// one window's compact level-0 rows as launch_obj_level0, from the pair's own interval; raymap[k] = pair_map[k] % R
void launch_inst_level0(const float* near_inst, const float* far_inst, const float* rays_d, const float* edges, const int* pair_map,
                        const int* count, int R, int N, float* t0_c, float* far_c, float* rays_d_c, int* raymap, hipStream_t s);
// missed pairs of the per-instance outputs (any may be null): rgb = white_bkgd ? 1 : 0, acc = depth = 0
void launch_inst_fill_misses(const float* near_inst, const float* far_inst, long pairs, int white_bkgd, float* rgb, float* acc,
                             float* depth, hipStream_t s);
// one window's compact results (composited WITHOUT white) to their pairs: prem_* (K R) keep them as they are, the per-instance
// outputs (any may be null) get rgb + (1 - acc) when white_bkgd - the arithmetic of k_composite's white background
void launch_inst_scatter(const int* pair_map, const int* count, int R, const float* rgb_c, const float* acc_c, const float* depth_c,
                         int white_bkgd, float* prem_rgb, float* prem_acc, float* prem_depth, float* rgb, float* acc, float* depth,
                         hipStream_t s);
// depth-ordered composite of a ray's hit instances (include/neo360_hip.h: COMPOSITE RECURRENCE); any output may be null
void launch_inst_composite(const float* near_inst, const float* far_inst, int K, int R, const float* prem_rgb, const float* prem_acc,
                           const float* prem_depth, int white_bkgd, float* rgb, float* acc, float* depth, int* instance_id,
                           hipStream_t s);

// edit.hip - edited render of neo_tp_render_edited (include/neo360_hip.h: EDIT RULE, LAYER RECURRENCE)
constexpr int TP_MAX_EDITS = 32;
struct TpEditTable {                 // per instance: density scale and rgb tint; travels by value as a kernel argument
    float scale[TP_MAX_EDITS];
    float tint[TP_MAX_EDITS][3];
};
// in place on (R,N,4) rows: the samples inside the closed interval of a hit pair (i, ray) are multiplied by instance i's scale /
// tint, i ascending; a sample inside no interval is not written.  K == 0 launches nothing.
void launch_tp_edit(float* rgbsigma, const float* t, const float* near_inst, const float* far_inst, int K, int R, int N,
                    const TpEditTable& tab, hipStream_t s);
// launch_composite mode 1 (t_row_stride N, no white background) with L <= 32 layers per ray: l_key, l_acc, l_depth (L,R), l_rgb
// (L,R,3); visibility (L,R) and every other output may be null; weights are the scene's own (k_composite's)
void launch_composite_layers(const float* rgbsigma, const float* t, const float* rays_d, const float* t_far, int R, int N,
                             const float* l_key, const float* l_rgb, const float* l_acc, const float* l_depth, int L, float* rgb,
                             float* acc, float* depth, float* weights, float* lambda, float* visibility, hipStream_t s);

// decompose.hip - per-instance layers of neo_tp_render_decomposed (include/neo360_hip.h: DECOMPOSITION RULE)
// (R,N,4) rows, positions and scene weights (k_composite mode 1's w_out) -> per owner slot 0 .. K (K = the rest): rgb (K+1,R,3),
// acc, depth (K+1,R), and id (R); bg_lambda (R) and every output may be null.  K <= 32, N <= 1024; K == 0 launches, R == 0 does not.
void launch_tp_decompose(const float* rgbsigma, const float* t, const float* weights, const float* near_inst, const float* far_inst,
                         int K, int R, int N, const float* bg_lambda, float* rgb, float* acc, float* depth, int* id, hipStream_t s);

// occupancy.hip - the occupancy grids of the NeO-360 and the vanilla scene (include/neo360_hip.h: OCCUPANCY GRID, KEEP RULE, BOX GRID)
// What the KEEP RULE (occ_points.h) does with a point outside the grid's box: the edge cell decides (the unit cube of the NeO-360
// scene), the point is kept, or the point is skipped (the vanilla box without and with `clip`).
enum { OCC_CLAMP = 0, OCC_KEEP = 1, OCC_SKIP = 2 };
// bits (GRID LAYOUT of occupancy.hip) or NULL for "no grid"; G^3 cells, cell = floor((x - lo) scale) per axis, scale formed once in
// host fp32 (occ_grid_unit / occ_grid_box); travels by value as a kernel argument
struct OccGrid {
    const uint32_t* bits;
    int G;
    float lo[3], scale[3];
    int outside;
};
// One launch's point rows, `cap` of them, in one buffer of occ_rows_bytes(cap) (march.h: launch_point_list fills them): row k is ONE
// point - the origin, direction and t of its ray, the view direction of its quirk-Q1 ray, dst = its place in the window's rows - and
// out its (rgb, sigma) row; iota = the identity map of the evaluator's compact launch; count the device word; totals the
// compaction's per-workgroup sums.  far: the ray's sphere exit, which only the outside-sphere evaluators read.
struct OccRows {
    float *out, *o, *d, *v, *t, *far;
    int *dst, *iota, *count, *totals;
    void carve(void* base, size_t cap);
};
size_t occ_rows_bytes(size_t cap);
void launch_occ_iota(int* map, int n, hipStream_t s);
// sigma (G probes)^3 activated densities -> G^3 / 32 words: any probe > threshold, dilation, unit-sphere clip (sphere = false: none)
void launch_occ_from_sigma(const float* sigma, int G, int probes, float threshold, int dilate, uint32_t* bits, hipStream_t s,
                           bool sphere = true);

}  // namespace neo
