/*
 * neo360_hip.h — C ABI of libneo360_hip.so, the MI355X (gfx950) implementation of
 * the NeO-360 ray-marching hot path.
 *
 * The reference (zubair-irshad/NeO-360) is pure Python/PyTorch and has no FFI of
 * its own; each entry point below replaces a reference *function* (cited as
 * file:line, paths relative to the reference root) at the granularity a
 * maintainer would bind with ctypes.
 *
 * Conventions
 *  - Plain C: pointers + sizes, no torch / C++ types.  `stream` is a hipStream_t
 *    passed as void* (NULL = default stream).
 *  - Unless marked [host], every pointer is a DEVICE pointer owned by the caller
 *    (e.g. a PyTorch-ROCm tensor's data_ptr()).  The library never frees caller
 *    memory and keeps no reference past the call, except neo_*_upload / set_*
 *    which copy / re-layout into context-owned buffers before returning
 *    (stream-ordered).
 *  - All tensors are dense, row-major fp32 unless stated.
 *  - Return value: 0 on success, negative neo_status otherwise (never throws).
 *    neo_last_error() gives a human-readable message for the calling thread.
 *  - No call synchronises the device; all work is enqueued on `stream`.
 *  - A context is bound to one device; calls on one context must not overlap
 *    from several host threads (same rule as the reference's nn.Module).
 */
#ifndef NEO360_HIP_H
#define NEO360_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct neo_ctx neo_ctx;

typedef enum {
    NEO_OK = 0,
    NEO_ERR_INVALID = -1,   /* bad argument (null pointer, unsupported size)  */
    NEO_ERR_HIP = -2,       /* a HIP runtime call failed (see neo_last_error) */
    NEO_ERR_STATE = -3,     /* weights / scene not uploaded yet               */
    NEO_ERR_NOMEM = -4
} neo_status;

/* ---- lifecycle -------------------------------------------------------- */
int neo_abi_version(void);                       /* bumps on any signature change */
const char* neo_last_error(void);
int neo_ctx_create(int device, neo_ctx** out);
int neo_ctx_destroy(neo_ctx* ctx);
/* Read-and-clear the device-side assertion word.  bit0 (NEO_FLAG_SPHERE_MISS): a ray missed the unit
 * sphere — the reference's AssertionError at models/neo360/helper.py:271,:426.  bit1 (NEO_FLAG_SPLIT_RANGE): an
 * operand of a split-fp16 kernel left the fp16 range (results of that call invalid; select precision 0).  bit2
 * (NEO_FLAG_SPLIT_STATIC, always together with bit1): the offending operand is a static one - packed weights or an
 * uploaded feature map - so every call on this (weights, scene) pair trips again: a read that returns bit1 re-arms the
 * one-time checks of static operands, here and in neo_ctx_take_flags.  The range has a low end: a linear layer whose
 * largest |w| is non-zero and below 2^-13 (vanilla, Mip-NeRF 360), 2^-11 (neo_tp_upload_mlp), 2^-9 (neo_pix_upload_mlp)
 * or 2^-6 (neo_enc_upload) raises bits 1 and 2 on the first split-fp16 launch after its upload (the hi/lo planes keep
 * too few bits of such weights; a layer folded into another one in fp64 at pack time is exempt), and so does an uploaded
 * feature map that a split kernel reads without the fp32 pre-projection when its largest |x| is non-zero and below 2^-8
 * (neo_tp_set_scene: the summed tri-planes in modes 0, 1 and in slots 0, 1 of mode 3, the latent in mode 0;
 * neo_pix_set_scene: the latent with pre-projection off).  The latent of neo_enc_floorplans is a per-call operand: below
 * 2^-6 it raises bit 1 alone.
 * Synchronises `stream`.  [flags: host out] */
#define NEO_FLAG_SPHERE_MISS 1u
#define NEO_FLAG_SPLIT_RANGE 2u
#define NEO_FLAG_SPLIT_STATIC 4u
int neo_ctx_poll_flags(neo_ctx* ctx, uint32_t* flags, void* stream);
/* The same read WITHOUT a synchronisation (what a caller's chunk loop wants: the reference's own loop makes 300
 * forward calls per frame, neo360/model.py:861-907).  post: enqueue on `stream` a copy of the word into a pinned host
 * slot + its clear + an event; returns at once.  take: OR of the posted reads that have completed (wait == 0), or of
 * all posted reads after waiting for their events (wait != 0); a read is reported once.  pending [host out, may be
 * NULL]: posted reads still in flight after the call.  Up to 64 reads may be outstanding; a post that finds all 64
 * still in flight posts nothing (the device word is sticky until a read clears it: a later read reports it, and
 * take(wait != 0) finishes with one synchronous read on `stream` in that case).  Neither post nor take(wait = 0)
 * ever blocks.  sync_count: how many blocking waits (stream / event synchronisations) the flag calls of this context
 * have issued so far - 0 for a loop of post + take(wait = 0). */
int neo_ctx_post_flags(neo_ctx* ctx, void* stream);
int neo_ctx_take_flags(neo_ctx* ctx, int wait, void* stream, uint32_t* flags, int* pending);
int neo_ctx_sync_count(neo_ctx* ctx, uint64_t* blocking_waits);
/* One context may be driven from several streams: its scratch (workspaces, per-launch tables, projected maps) is shared,
 * so every rendering / evaluator / backward call on a stream other than the previous call's first waits - on the
 * device, hipStreamWaitEvent, never on the host - for an event recorded behind that previous call.  stream_waits:
 * how many such cross-stream waits this context has inserted (0 for the usual one-stream caller). */
int neo_ctx_stream_waits(neo_ctx* ctx, uint64_t* cross_stream_waits);
/* Scratch lanes (round 6).  The reference drives the module as 300 calls of 1024 rays per frame (render_rays_test,
 * neo360/model.py:861-907); launched back to back on one stream every call ends on a partly filled machine (2,064 tiles
 * of a coarse launch on 512 workgroup slots).  A context therefore owns FOUR sets of render scratch (grown on first use): neo_ctx_set_lane
 * picks the set the next calls use (0, the default, .. 3).  neo_tp_render writes its lane's scratch only and reads the shared
 * weights / maps, so two renders on different lanes AND different streams are not ordered against each other and overlap
 * on the device; every other entry point (uploads, set_scene, evaluator / training calls) stays ordered against all
 * earlier calls of the context, on any lane.  A one-lane, one-stream caller sees no difference. */
int neo_ctx_set_lane(neo_ctx* ctx, int lane);
/* Pixel-grid hint for whole-frame renders (round 6).  When the rays handed to the next neo_tp_render calls are the pixels of a
 * row-major image `width` wide (ray 0 of a call = pixel `first_ray` of the frame: a rank's shard starts in the middle), the
 * evaluators visit the rays of every whole band of image rows in small pixel patches (2 x 2 inside the unit sphere, 8 x 8 outside)
 * instead of row by row: the workgroups resident on an XCD then cover a compact piece of the image and share feature texels in that
 * XCD's L2 in both image directions - fabric-side traffic of a full-frame launch 59.8 -> 41.7 GB inside, 11.6 -> 1.8 GB outside
 * (profiles/r06_ray_patch_order.log).  Pure scheduling: every output value is bitwise the one without the hint.  width = 0
 * (default) removes it; width must be a multiple of 8.  The reference has no counterpart (its chunk loop renders 1024 consecutive
 * rays at a time; datasets/ray_utils.py:96-104 defines the row-major order). */
int neo_ctx_set_ray_grid(neo_ctx* ctx, int width, long first_ray);
/* Quad order of the NeO-360 pre-projected split evaluators.  A 64-point tile normally holds 64 consecutive samples of one ray; in
 * quad order it holds 64 / G samples of G consecutive rays of the launch (G = 4, a quad: with the pixel-grid hint a 2 x 2 pixel patch
 * inside the unit sphere, four adjacent pixels of a patch row outside; without it four consecutive rays of the caller; G = 8 / 16:
 * two / four such quads), so that the four rows behind one gather instruction are neighbouring rays at one sample index and fall
 * on almost the same texels.  Pure scheduling: every output value is bitwise the one of the ray-major order.  mode -1 (default): the
 * library's per-launch choice (api_tp.hip:tp_launch; $NEO_TP_QUAD, read once, replaces that choice: 0, 1 or a group size); 0:
 * ray-major everywhere; 1: quads of four in every launch that can take them (compact launches - culled background, objects,
 * instances - never do); 4 / 8 / 16: that many rays per group everywhere (4 is 1).  The setter wins over the environment variable. */
int neo_ctx_set_tp_quad(neo_ctx* ctx, int mode);

/* Arithmetic of the per-point MLP GEMMs of every renderer (vanilla, NeRF_TP, Mip-NeRF 360, PixelNeRF).
 * 1 (the context default, and the default of the Python modules, "f16x3"): fp16 MFMA with every fp32
 * operand split into hi+lo fp16 and three products per term (a_hi b_hi + a_hi b_lo + a_lo b_hi, fp32
 * accumulate) - fp32-class error at a 5.3x higher matrix-pipe ceiling; operands must stay below the fp16
 * range (|x| < 65504: checked, see NEO_FLAG_SPLIT_RANGE).  0 ("f32"): exact fp32 MFMA
 * (v_mfma_f32_32x32x2_f32), no range limit.  Both meet the 1e-4 parity contract. */
int neo_ctx_set_precision(neo_ctx* ctx, int mode);

/* torch.linspace(start, end, steps) for fp32 on the host (symmetric fill,
 * step=(end-start)/(steps-1)) — the constant tables the samplers start from
 * (vanilla_nerf/helper.py:425, :589; neo360/helper.py:36, :197).  No GPU needed.
 * out [host]. */
void neo_linspace_host(float start, float end, int steps, float* out);

/* ---- ray generation ---------------------------------------------------- */
/* datasets/ray_utils.py:84-104 get_ray_directions + :133-176 get_rays
 * (output_view_dirs=True, output_radii=True).  c2w [host]: 12 floats, row-major
 * 3x4.  Outputs (H*W,3),(H*W,3),(H*W,3),(H*W); rays_d == viewdirs (the
 * reference aliases them); radii may be NULL. */
int neo_raygen(neo_ctx* ctx, int H, int W, float focal, const float* c2w,
               float* rays_o, float* viewdirs, float* rays_d, float* radii, void* stream);

/* datasets/ray_utils.py:17-68 == models/neo360/helper.py:275-323
 * bbox_intersection_batch: float64 slab test, rays already in the box frame.
 * bounds [host]: 6 doubles (min xyz, max xyz).  hit: uint8 0/1 (bit-exact
 * contract); tmin/tmax: doubles, 0 where missed; either may be NULL. */
int neo_aabb_intersect(neo_ctx* ctx, const double* bounds, const double* rays_o,
                       const double* rays_d, int R, uint8_t* hit, double* tmin,
                       double* tmax, void* stream);

/* The same for rays [ray0, ray0 + n_rays) of the row-major H x W frame, written to rows [0, n_rays) of the
 * outputs: a rank of a ray-sharded render (models/interface.py:30-50 gathers the pieces) generates only its range. */
int neo_raygen_range(neo_ctx* ctx, int H, int W, float focal, const float* c2w, int ray0, int n_rays,
                     float* rays_o, float* viewdirs, float* rays_d, float* radii, void* stream);

/* models/neo360/helper.py:359-373 sample_rays_in_bbox over n_boxes oriented boxes: per box the rays are moved to
 * the box frame in float64 (:325-331; world_to_box [host]: n_boxes x 16 doubles, the row-major 4x4
 * np.linalg.inv([R|T]) the caller computes as get_object_rays_in_bbox does, :348-357), slab-tested (:275-323;
 * bounds [host]: n_boxes x 6 doubles, min xyz then max xyz), tmin/tmax rounded to float32, and merged by the
 * running minimum that treats 0 as "no hit".  rays_o / rays_d: (R,3) float64.  Outputs (any may be NULL):
 * hit_per_box (n_boxes,R) uint8, near (R) / far (R) float32 merged, mask (R) uint8 = near != 0 && far != 0
 * (bit-exact contract). */
int neo_aabb_multi(neo_ctx* ctx, int n_boxes, const double* world_to_box, const double* bounds,
                   const double* rays_o, const double* rays_d, int R, uint8_t* hit_per_box, float* near,
                   float* far, uint8_t* mask, void* stream);

/* models/neo360/helper.py:375-394 sample_rays_in_bbox_list: the same box-frame transform and slab test as neo_aabb_multi, with the
 * interval of EVERY box kept instead of the merged one.  Outputs (any may be NULL): near (n_boxes,R) / far (n_boxes,R) float32 =
 * tmin / tmax rounded to float32, 0 where the ray misses the box (the reference's "no hit" sentinel); hit (n_boxes,R) uint8
 * (bit-exact contract; the hit_per_box of neo_aabb_multi). */
int neo_aabb_per_box(neo_ctx* ctx, int n_boxes, const double* world_to_box, const double* bounds,
                     const double* rays_o, const double* rays_d, int R, float* near, float* far, uint8_t* hit,
                     void* stream);

/* models/neo360/helper.py:253-273 intersect_sphere.  far (R); ok (R) uint8 =
 * (1-|p|^2 >= 0), may be NULL; a miss also raises flag bit0. */
int neo_intersect_sphere(neo_ctx* ctx, const float* rays_o, const float* rays_d, int R,
                         float* far, uint8_t* ok, void* stream);

/* ---- stage-level operators (stage-isolated parity) ---------- */
/* helper.py pos_enc (neo360/helper.py:121-125 == vanilla_nerf/helper.py:445-449):
 * x (n,C) -> out (n, C*(2*(max_deg-min_deg)+1)). */
int neo_pos_enc(neo_ctx* ctx, const float* x, int n, int C, int min_deg, int max_deg,
                float* out, void* stream);

/* sorted_piecewise_constant_pdf + sample_pdf's sort
 * (vanilla_nerf/helper.py:567-616, neo360/helper.py:174-231), randomized=False.
 * t_prev (R,n_prev), weights (R,n_prev): bins are the n_prev-1 midpoints of
 * t_prev, pdf weights are weights[:,1:-1] (the slicing the callers do at
 * vanilla_nerf/model.py:171-175, neo360/model.py:308-318).  t_out
 * (R, n_prev+n_new) sorted ascending, or descending when `descending` != 0
 * (the background branch's flip, neo360/helper.py:234-239). */
int neo_resample(neo_ctx* ctx, const float* t_prev, const float* weights, int R, int n_prev,
                 int n_new, int descending, float* t_out, void* stream);

/* volumetric_rendering.  mode 0: vanilla (vanilla_nerf/helper.py:521-559);
 * mode 1: NeO-360 inside sphere (neo360/helper.py:128-171, in_sphere=True,
 * needs t_far (R)); mode 2: NeO-360 outside sphere (t descending).
 * rgbsigma (R,N,4) = (r,g,b,sigma); t (R,N); rays_d (R,3).
 * Outputs: rgb (R,3), acc (R), depth (R), weights (R,N), lambda (R) [mode 1];
 * any output may be NULL. */
int neo_composite(neo_ctx* ctx, int mode, const float* rgbsigma, const float* t,
                  const float* rays_d, const float* t_far, int R, int N, int white_bkgd,
                  float* rgb, float* acc, float* depth, float* weights, float* lambda,
                  void* stream);

/* ---- vanilla NeRF (models/vanilla_nerf/model.py) -------------------------- */
/* Upload one NeRFMLP (vanilla_nerf/model.py:44-98).  slot 0 = coarse_mlp,
 * 1 = fine_mlp.  weights/biases [host arrays of 12 device pointers], order:
 * pts_linears.0..7, views_linear.0, bottleneck_layer, density_layer, rgb_layer;
 * torch.nn.Linear layout (out,in).  Re-packed on the device into the MFMA
 * fragment order; the caller's tensors are not referenced afterwards. */
int neo_vanilla_upload_mlp(neo_ctx* ctx, int slot, const float* const* weights,
                           const float* const* biases, void* stream);

/* pos_enc + NeRFMLP.forward + activations for R*N points
 * (vanilla_nerf/model.py:183-204): points o + t*dirs; t is (R,N) when
 * t_row_stride == N, or one shared row when t_row_stride == 0.
 * out (R,N,4) = (rgb after sigmoid+padding, sigma after softplus(raw-1)). */
int neo_vanilla_mlp(neo_ctx* ctx, int slot, const float* rays_o, const float* dirs,
                    const float* t, int t_row_stride, int R, int N, float* out, void* stream);

/* NeRF.forward (vanilla_nerf/model.py:154-216), randomized=False, both levels.
 * Samples are cast along `viewdirs`, compositing scales by |rays_d| (as the
 * reference).  Per level l: rgb_l (R,3), acc_l (R), depth_l (R); level-0
 * outputs may be NULL. */
int neo_vanilla_render(neo_ctx* ctx, const float* rays_o, const float* viewdirs,
                       const float* rays_d, int R, float near, float far, int n_coarse,
                       int n_fine, int white_bkgd, float* rgb0, float* acc0, float* depth0,
                       float* rgb1, float* acc1, float* depth1, void* stream);

/* VANILLA MARCHING FRAME: empty-space skipping and early ray termination for the vanilla renderer.  A vanilla NeRF is fitted to ONE
 * scene, its density depends on the position alone and it has no outside-sphere half, so a grid built once from its own density
 * stays valid for every later frame and both savings apply to the whole frame.  The pieces are those of the NeO-360 frame further
 * down in this header (OCCUPANCY GRID, KEEP RULE, STOP RULE, ACCELERATED FRAME), restated for a grid over a box and for composite
 * mode 0.
 *
 * COMPACT EVALUATOR LAUNCH.  neo_vanilla_mlp_compact is neo_vanilla_mlp on single points whose number lives on the device: rays_o,
 * dirs (cap,3), t (cap) and out (cap,4) are allocated for `cap` rows, the host's bound, and min(*count_dev, cap) of them are live
 * (count_dev [device]: one int; 0 is a valid launch).  Row k is the point rays_o[k] + t[k] * dirs[k] seen along dirs[k].  Its out row
 * is bitwise what neo_vanilla_mlp gives the same point, whatever its neighbours and whichever kernel variant runs; the variant is
 * chosen from the process's settings, never from the count.  A row at or behind the count is neither read nor written and takes no
 * part in the fp16 range check; a workgroup whose first row is at or behind the count leaves before its first barrier. */
int neo_vanilla_mlp_compact(neo_ctx* ctx, int slot, const float* rays_o, const float* dirs, const float* t, int cap,
                            const int* count_dev, float* out, void* stream);

/* BOX GRID.  G^3 cells over a caller-given box [lo_a, hi_a) per axis (lo, hi [host]: 3 floats each, finite, lo_a < hi_a); G and the
 * bit layout are the OCCUPANCY GRID's.  scale_a = (float)G / (hi_a - lo_a) is formed ONCE, on the host, in fp32 (one subtraction,
 * one division).  The cell of a coordinate x_a, in fp32 on the device: c_a = floorf((x_a - lo_a) * scale_a) - one subtraction, one
 * multiply.  A point is OUTSIDE iff some c_a < 0 or c_a >= G (compared as floats; an overflow to infinity is outside) - the
 * unit-cube rule clamps instead, which is not enough here, because vanilla samples run to `far` whatever the box is.
 * BOX KEEP RULE.  Sample j of ray r, at x = rays_o[r] + t[r][j] * viewdirs[r] (one fp32 multiply and one fp32 add per coordinate,
 * the evaluator's own expression), is KEPT iff a coordinate of x is not finite (written as the negation of |x| < inf, so that a NaN
 * survives to the caller), or there is no grid, or x is outside and clip == 0, or x is inside and the bit of (c_0, c_1, c_2) is set.
 * With clip != 0 a point outside the box is skipped.
 *
 * neo_vanilla_set_occupancy copies `bits` [device, G^3 / 8 bytes] into context-owned memory and records the box and `clip`; it is
 * ordered behind every earlier call of the context.  bits == NULL removes the grid.  The grid belongs to the uploaded weights,
 * which the library cannot check: install a new one after an upload.  neo_vanilla_set_march_window: rays per window of
 * neo_vanilla_render_marching, 1 .. 65536, 0 = the default (8192); a window bounds the extra workspace at 68 bytes per (ray,
 * sample) of one window and segment.  Results do not depend on it. */
int neo_vanilla_set_occupancy(neo_ctx* ctx, const uint32_t* bits, int G, const float* lo, const float* hi, int clip, void* stream);
int neo_vanilla_set_march_window(neo_ctx* ctx, int rays);

/* The BOX KEEP RULE on caller rows: rays_o, dirs (R,3), t (R,N) -> keep (R,N) uint8 0 / 1.  bits [device] may be NULL (no grid: all
 * ones; G, lo, hi and clip are then not read).  R == 0 is a valid call.  Touches no context-owned memory. */
int neo_vanilla_occupancy_keep(neo_ctx* ctx, const uint32_t* bits, int G, const float* lo, const float* hi, int clip,
                               const float* rays_o, const float* dirs, const float* t, int R, int N, uint8_t* keep, void* stream);

/* neo_occupancy_from_sigma (below) without its last step, the unit-sphere clip: the lattice is the box's, and a box has no sphere. */
int neo_occupancy_from_sigma_box(neo_ctx* ctx, const float* sigma, int G, int probes, float threshold, int dilate, uint32_t* bits,
                                 void* stream);

/* MODE-0 STOP RULE: the STOP RULE (below) restated for neo_composite mode 0.  delta_i = t_{i+1} - t_i, the last one 1e10, each
 * times |rays_d| (the norm of rays_d, not of viewdirs); alpha = alpha(sigma * delta); keep = (1 - alpha) + 1e-10f; the 64-lane
 * inclusive product scan in fp64; carry *= the round's last lane.  These are mode 0's own lines, so at a boundary b that is a
 * multiple of 64, (float)carry_b is the transmittance that the composite assigns to sample b, bit for bit.  Segment 0 is always
 * marched.  Segment k >= 1 is marched iff no earlier boundary b had (float)carry_b < eps - a negation, so a NaN marches on.
 * `segment` is a positive multiple of 64, eps lies in [0, 1).  stop (R) int32 = the leading samples marched: N or a boundary;
 * trans (R) = (float)carry at the stop.  R == 0 is a valid call.  Touches no context-owned memory. */
int neo_vanilla_termination_stops(neo_ctx* ctx, const float* rgbsigma, const float* t, const float* rays_d, int R, int N, float eps,
                                  int segment, int* stop, float* trans, void* stream);

/* neo_vanilla_render in which a sample is evaluated iff the BOX KEEP RULE of the installed grid keeps it AND it lies in front of the
 * ray's stop.  A sample that is not evaluated has the row (0, 0, 0, 0), to which composite mode 0 gives weight exactly 0 and an
 * unchanged product (alpha(0 * delta) = 0, also for the last delta 1e10, and 1.0f + 1e-10f == 1.0f).  An evaluated sample goes through
 * the compact evaluator launch and is bitwise neo_vanilla_render's for its position.  The composites, the resampling (on the resulting
 * level-0 weights) and white_bkgd are neo_vanilla_render's.
 * LEVELS.  Level 1 follows the MODE-0 STOP RULE, applied to its rows in which the samples that are not kept are zero.  Level 0 follows
 * it only with coarse != 0, which moves the level-1 positions: NO bound is claimed for that mode.  A level that does not follow the rule
 * has stop = N; with no grid either it is the dense launch of neo_vanilla_render.  eps == 0 stops nothing.  use_grid == 0 ignores an
 * installed grid.  Without a grid (or with every cell set, or with a box that holds no sample and clip == 0) at eps == 0 the six
 * outputs are bitwise neo_vanilla_render's.
 * BOUND (coarse == 0, level 1), against the same call at eps == 0 with the same grid.  Level 0, and therefore the level-1 positions and
 * the keep masks, are identical in the two calls; a ray that never stops is bitwise equal.  Let a ray stop at b with L = (float)carry_b
 * < eps, the `trans` of neo_vanilla_termination_stops, and let F >= 0 be its final transmittance in the other call.  With T_{i+1} =
 * T_i (1 - alpha_i + 1e-10), a weight is w_i = alpha_i T_i = T_i - T_{i+1} + 1e-10 T_i, so the skipped weights sum to S = L - F +
 * 1e-10 sum T_i <= (1 + 1024e-10) L.  Colours lie in (-0.001, 1.001): without white_bkgd the change is -sum_skipped w_i c_i, at
 * most 1.001 S; with it every sample contributes w_i (c_i - 1) instead - the white term turns c into 1 - c - and |c_i - 1| < 1.001
 * again.  Either way |rgb change| < 1.0011 L per channel in real arithmetic, the same constant as for the NeO-360 rule; the asserted
 * 1.003 L leaves 0.0019 L for the fp32 rounding of the two sums being compared.  Depth: positions are <= far, so |depth change| <=
 * far S <= 1.0000002 far L, asserted as 1.001 far L.
 * Per window of rays and per segment: compact the alive rays on their transmittance, classify and compact their samples of the
 * segment, one compact evaluator launch, scatter into zero-filled rows, advance the product.  No call synchronises the device; the
 * only atomic is the range guard's flag word.
 * samples0 / samples1 (may be NULL, and any pointer in them): the level's positions t (level 0: ONE row of N_0, shared by all rays;
 * level 1: (R,N_1)), weights w (R,N), keep (R,N) uint8 - the BOX KEEP RULE on the WHOLE row, behind the stop as well, all ones
 * without a grid - stop (R) int32 and rows (R,N,4).  The evaluated set is keep & (j < stop).  kept (may be NULL): int64[2] on the
 * device, the evaluated samples per level; nothing is read back. */
typedef struct { float* t; float* w; uint8_t* keep; int* stop; float* rows; } neo_vanilla_march_samples;
int neo_vanilla_render_marching(neo_ctx* ctx, const float* rays_o, const float* viewdirs, const float* rays_d, int R, float near,
                                float far, int n_coarse, int n_fine, int white_bkgd, float eps, int segment, int coarse, int use_grid,
                                float* rgb0, float* acc0, float* depth0, float* rgb1, float* acc1, float* depth1,
                                const neo_vanilla_march_samples* samples0, const neo_vanilla_march_samples* samples1, long long* kept,
                                void* stream);

/* VANILLA MARCHING TRAINING: the pieces between neo_vanilla_mlp_train_forward / _backward (further down: they work on arbitrary rows,
 * each with its own cond) and the BOX GRID above, so that a training step evaluates - forward and backward - only the samples the
 * grid keeps, and the grid follows the weights while they move.  No stop rule: a training ray sees its whole interval.
 *
 * ROW BUILDER.  neo_vanilla_train_rows: the grid as neo_vanilla_occupancy_keep takes it (bits == NULL: no grid; G, lo, hi, clip are
 * then not read), rays_o, dirs (R,3), t (R,N), dir_enc (R,27), and `cap`, the rows index / x_enc / cond are allocated for.
 * keep (R,N) uint8 = the BOX KEEP RULE, bitwise neo_vanilla_occupancy_keep's.  count [device]: one int = the kept samples of the
 * whole call, NOT clamped to cap.  For k < min(count, cap), in ascending flat order: index[k] = r N + j of the k-th kept sample;
 * x_enc[k] (63) = the encoding of x = rays_o[r] + t[r][j] * dirs[r] (one fp32 multiply, one fp32 add), bitwise what
 * neo_pos_enc(x, 3, 0, 10) gives that point; cond[k] (27) = dir_enc[r].  Rows at or behind the count are neither read nor written.
 * R == 0 (count = 0) and a count of 0 are valid.  Two launches (classify + per-workgroup totals, then rank + emit: the compaction of
 * the marching frames); no atomics, nothing synchronises, and the outputs do not depend on the launch geometry.  The totals live
 * in a grow-only workspace of the context (4 bytes per 1024 samples), so the call is ordered like every call that writes one.
 *
 * ACTIVATE AND SCATTER.  neo_vanilla_train_scatter: raw_rgb (K,3), raw_sigma (K), index (K) - distinct values in [0, P) - noise (P)
 * or NULL, noise_scale -> packed (P,4): row index[k] is bitwise neo_tp_activate's row for (raw_rgb[k], raw_sigma[k],
 * noise[index[k]]); every other row is (0, 0, 0, 0), to which composite mode 0 gives weight exactly 0 and an unchanged product (see
 * neo_vanilla_render_marching).  An index outside [0, P) writes nothing.  neo_vanilla_train_scatter_backward gathers
 * g_packed[index[k]] and returns g_rgb (K,3), g_sigma (K), bitwise neo_tp_activate_backward on those rows.  K is a host value in both
 * (0 <= K <= P); K == 0 launches nothing that reads a row (the forward still zero-fills packed).
 *
 * PROBE POINTS.  neo_vanilla_grid_probes: pts (G^3,3) in the grid's [ix][iy][iz] order, ONE point per cell of the BOX GRID over
 * [lo, hi).  Per axis a, with w_a = (hi_a - lo_a) / (float)G formed once on the host in fp32: x_a = lo_a + ((float)c_a + u_a) * w_a
 * (one add, one multiply, one add in fp32), u_a in [0, 1) = the value neo_rand_uniform gives key `seed` at row = the cell's linear
 * index, col = `step`, stream_id = 8 + a (streams 0..7 belong to the samplers; the Philox counter is (cell, step, 8 + a, 0)).
 * CONTRACT: the point of cell (c_0, c_1, c_2) lies in that cell under the BOX GRID's own fp32 expression floorf((x_a - lo_a) *
 * scale_a).  A candidate x_a that rounding pushed over a face - its own cell expression is not c_a - is PULLED BACK to the centre
 * of that axis, lo_a + ((float)c_a + 0.5f) * w_a; the other two coordinates stay.  So that the centre itself is inside, a box whose
 * cell is thinner than 64 ulp of its largest coordinate (w_a * 2^17 < max(|lo_a|, |hi_a|)) is refused.  The same (seed, step)
 * gives the same bits.
 *
 * RUNNING DENSITY.  neo_vanilla_density_update: density (G^3) in place = max(decay * density, max(sigma0, sigma1)) per cell, sigma1
 * may be NULL; decay in [0, 1]; a NaN on either side of a max gives NaN, which neo_occupancy_from_sigma_box(density, G, probes = 1,
 * threshold, dilate, bits) - the one threshold kernel - treats as occupied. */
int neo_vanilla_train_rows(neo_ctx* ctx, const uint32_t* bits, int G, const float* lo, const float* hi, int clip, const float* rays_o,
                           const float* dirs, const float* t, const float* dir_enc, int R, int N, int cap, uint8_t* keep, int* count,
                           int* index, float* x_enc, float* cond, void* stream);
int neo_vanilla_train_scatter(neo_ctx* ctx, const float* raw_rgb, const float* raw_sigma, const int* index, long K, const float* noise,
                              float noise_scale, long P, float* packed, void* stream);
int neo_vanilla_train_scatter_backward(neo_ctx* ctx, const float* raw_rgb, const float* raw_sigma, const int* index, long K,
                                       const float* noise, float noise_scale, long P, const float* g_packed, float* g_rgb,
                                       float* g_sigma, void* stream);
int neo_vanilla_grid_probes(neo_ctx* ctx, int G, const float* lo, const float* hi, uint64_t seed, uint32_t step, float* pts,
                            void* stream);
int neo_vanilla_density_update(neo_ctx* ctx, float* density, const float* sigma0, const float* sigma1, int G, float decay, void* stream);

/* ---- NeO-360 decoder (models/neo360/model.py NeRF_TP) ---------------------- */
/* Upload one NeRFPPMLP (neo360/model.py:37-108).  slot 0..3 = fg_coarse,
 * fg_fine, bg_coarse, bg_fine.  input_ch = 3 (fg) or 4 (bg).  weights/biases
 * [host arrays of 9 device pointers], order: pts_linears.0..3,
 * views_linear.0, views_linear.1, bottleneck_layer, density_layer, rgb_layer. */
int neo_tp_upload_mlp(neo_ctx* ctx, int slot, int input_ch, const float* const* weights,
                      const float* const* biases, void* stream);

/* Scene features = the encoder outputs the reference recomputes per chunk
 * (neo360/model.py:272-274).  planes: 3 x (NV,Cw,Hp,Wp) NCHW; latent
 * (NV,Cl,Hf,Wf) NCHW; re-laid out channels-last into context-owned buffers.
 * Cw must be 128 and Cl 512 (the reference's fixed widths). */
int neo_tp_set_scene(neo_ctx* ctx, const float* plane_xz, const float* plane_xy,
                     const float* plane_yz, int NV, int Cw, int Hp, int Wp,
                     const float* latent, int Cl, int Hf, int Wf, float image_w,
                     float image_h, void* stream);

/* Both arithmetic modes (the exact fp32 evaluator gathers the same projected maps since round 4; in it modes 2 and 3 both
 * project the planes for every slot).  A fresh context is in mode 3.  enable != 0: the 512-channel latent is pre-projected once per
 * (scene, MLP slot) through the local columns of pts_linears.0 and of pts_linears.3's skip half
 * (W . bilerp(F) = bilerp(W . F): neo360/model.py:110-158 is linear in the latent up to the first ReLU), and
 * the evaluator gathers the 256-channel result; costs 1 KB per latent texel and slot of context memory.
 * enable == 0: the latent itself is gathered and multiplied per point (the reference's operation order).
 * enable == 2: the three tri-planes are pre-projected the same way through the world columns (the 128-channel plane
 * sum of encoder_tp_fusion_conv.py:180-206 enters pts_linears.0 / .3 linearly too, model.py:123-137): no per-point world
 * GEMM stage, four 256-channel maps are gathered, blended and added; 1 KB per plane texel and slot on top.
 * enable == 3: as 2 for the outside-sphere slots 2, 3 (most of their samples lie outside every map: few taps, the GEMM stage
 * is pure saving), as 1 for the inside-sphere slots 0, 1 (every map carries weight: the larger taps cost more than the GEMM
 * stage they replace).  The Python modules default to 3. */
int neo_tp_set_preproject(neo_ctx* ctx, int enable);

/* `predict` + the feature lookups for one region at given sample positions
 * (neo360/model.py:343-464): slot 0/1 inside the sphere (tvals = t, ascending),
 * slot 2/3 outside (tvals = inverse radius, descending; needs far (R) from
 * neo_intersect_sphere).  tvals (R,N); out (R,N,4) = (rgb, sigma) after activations.
 * `chunk`, src_poses [host], focal/cx/cy as for neo_tp_render. */
int neo_tp_mlp(neo_ctx* ctx, int slot, const float* rays_o, const float* rays_d,
               const float* viewdirs, const float* tvals, const float* far, int R, int N,
               int chunk, const float* src_poses, int NV, float focal, float cx, float cy,
               float* out, void* stream);

/* NeRF_TP.forward decoder half (neo360/model.py:276-581), randomized=False,
 * out_depth=True semantics, for R rays processed in reference-sized chunks
 * (`chunk` rays per forward call: the view-direction tiling of
 * neo360/model.py:357-360 makes results depend on chunk membership).
 * src_poses [host]: NV*16 floats (c2w 4x4 row-major); focal/cx/cy: source view
 * 0's intrinsics (neo360/model.py:242-244).  Outputs per level l (any may be
 * NULL): rgb_l (R,3), fg_rgb_l (R,3), bg_rgb_l (R,3), fg_acc_l (R),
 * bg_lambda_l (R), depth_l (R).  A level struct may itself be NULL.  When
 * level0 is NULL, or none of its rgb / fg_rgb / bg_rgb / depth is set, the
 * coarse level is evaluated for its densities alone (they place the fine
 * samples): the pre-projected split evaluators skip its colour branch.  Level 1
 * is bitwise the same either way. */
typedef struct {
    float* rgb; float* fg_rgb; float* bg_rgb; float* fg_acc; float* bg_lambda; float* depth;
} neo_tp_level_out;
int neo_tp_render(neo_ctx* ctx, const float* rays_o, const float* rays_d,
                  const float* viewdirs, int R, int chunk, const float* src_poses, int NV,
                  float focal, float cx, float cy, int n_coarse, int n_fine, int white_bkgd,
                  const neo_tp_level_out* level0, const neo_tp_level_out* level1, void* stream);

/* The per-ray EXTRAS of a NeO-360 ray's whole interval histogram, inside and outside the unit sphere together, as DISTANCES ALONG THE
 * RAY: the unit of the ray parameter t of o + t d, which is the unit of the reference's fg_depth (and not that of its comp_depth =
 * fg_depth + bg_lambda * bg_depth, neo360/model.py:523, which adds a sum of weights times inverse radii to a distance).
 * Inputs per ray (all fp32, device): fg_t (R,N) ascending, fg_w (R,N), far (R) = the sphere exit of neo_intersect_sphere; bg_s (R,N)
 * descending inverse radius in [0, 1], bg_w (R,N), lambda (R) = the inside composite's last transmittance (bg_lambda); rays_o,
 * rays_d (R,3).  bg_s = bg_w = lambda = NULL selects the INSIDE-ONLY histogram (N intervals ending at far: the rows of
 * neo_tp_render_objects with far = far_obj); giving only some of the three is an error.  1 <= N <= 1024.
 * HISTOGRAM, M = 2 N intervals in ray order: inside interval i spans [fg_t[i], fg_t[i+1]] with fg_t[N] := far and has mass fg_w[i];
 * outside interval j spans, in inverse radius, [bg_s[j], bg_s[j+1]] with bg_s[N] := 0 (the reference's 1e10 last step: the last
 * interval runs out to infinite radius) and has mass lambda * bg_w[j].  The edge at inverse radius s lies at the distance
 * tau(s) = d1 + sqrt(max(1 / s^2 - rho2, 0)) / |d| with d1 = -(o.d) / |d|^2 and rho2 = |o + d1 d|^2 (|o + t d| = 1 / s); tau(0) = +inf
 * and tau(1) is the sphere exit, so the histogram is continuous there.  Knots c_0 = 0, c_{k+1} = c_k + m_k: no renormalisation, no clamp.
 * Everything is fp64 from the fp32 inputs and each output entry is rounded to fp32 once; no atomics, results repeat bit for bit.
 * Outputs, any of which may be NULL:  opacity (R) = c_M;  disparity (R) = sum_k m_k (1 / a_k + 1 / b_k) / 2 over the interval ends
 * as distances, 1 / inf = 0 (the expected DISPARITY on purpose: the last outside interval ends at infinity and usually holds the
 * remaining transmittance, so an expected distance is infinite on every ray that sees sky);  dist_pct (R, n_u) for u (n_u) [device]
 * ascending quantiles in [0, 1], 0 <= n_u <= 8: +inf when u >= c_M (the ray leaves), otherwise with c_k <= u < c_{k+1} and
 * off = (u - c_k) / m_k: inside a + off (b - a), outside tau(s_j + off (s_{j+1} - s_j)) - linear in inverse radius.
 * R == 0 is a valid call.  Touches no context-owned memory. */
int neo_tp_extras(neo_ctx* ctx, const float* fg_t, const float* fg_w, const float* far, const float* bg_s, const float* bg_w,
                  const float* lambda, const float* rays_o, const float* rays_d, int R, int N, const float* u, int n_u,
                  float* opacity, float* disparity, float* dist_pct /* (R, n_u) */, void* stream);

/* neo_tp_render with those extras per level, from the rows the call already has on the device (far from its own sphere intersection,
 * lambda = bg_lambda of the level): u (n_u) [device] as above, one struct per level; a struct, and any pointer in it, may be NULL.
 * neo_tp_render IS this call with u = NULL, n_u = 0 and both structs NULL: then the launches, the workspaces and every output are
 * what they always were.  A level whose extras are asked for has its two composites write their weights too (level 1: two more
 * lane workspaces of R x N floats) and one more small launch after its merge; the six outputs per level do not change. */
typedef struct { float* opacity; float* disparity; float* dist_pct; } neo_tp_extras_out;   /* (R), (R), (R, n_u) */
int neo_tp_render_extras(neo_ctx* ctx, const float* rays_o, const float* rays_d,
                         const float* viewdirs, int R, int chunk, const float* src_poses, int NV,
                         float focal, float cx, float cy, int n_coarse, int n_fine, int white_bkgd,
                         const neo_tp_level_out* level0, const neo_tp_level_out* level1, const float* u, int n_u,
                         const neo_tp_extras_out* extras0, const neo_tp_extras_out* extras1, void* stream);

/* The same render with BACKGROUND CULLING (opt-in).  The composite is rgb = fg_rgb + bg_lambda * bg_rgb and depth = fg_depth +
 * bg_lambda * bg_depth, bg_lambda being the foreground's final transmittance, and nothing in a ray's background half feeds
 * its foreground half.  The foreground of BOTH levels is therefore finished first; a ray survives iff
 * !(bg_lambda_0 < eps) || !(bg_lambda_1 < eps) (a NaN survives); the survivors are compacted in ascending ray order
 * (deterministic) and background level 0, its resampling and background level 1 run on them only.
 * Bound: bg_rgb is a sum of weights (<= 1 up to the 1e-10 terms of the transmittance product) times colours in
 * (-0.001, 1.001), bg_depth a sum of weights times inverse radii in [0, 1]; dropping a ray's background changes its rgb by
 * less than 1.002 * bg_lambda and its depth by less than 1.001 * bg_lambda, at either level (both lambdas are below eps).
 * A surviving ray's six outputs per level are bitwise those of neo_tp_render (the quirk-Q1 direction index is taken from the
 * ray's own index and R); a culled ray gets rgb = fg_rgb, bg_rgb = 0, depth = fg_depth at both levels; fg_rgb, fg_acc and
 * bg_lambda are neo_tp_render's for every ray.  Sphere-miss assertions cover every ray.  A culled ray's background is not
 * evaluated, so it takes no part in the fp16 range check of the split arithmetic either.
 * eps in (0, 1).  survivors_out [device, may be NULL]: receives the number of surviving rays; the call never reads it on the
 * host and synchronises nothing (the background launches are sized for R rays and take their row count from the device). */
int neo_tp_render_culled(neo_ctx* ctx, const float* rays_o, const float* rays_d,
                         const float* viewdirs, int R, int chunk, const float* src_poses, int NV,
                         float focal, float cx, float cy, int n_coarse, int n_fine, int white_bkgd,
                         const neo_tp_level_out* level0, const neo_tp_level_out* level1, float eps,
                         int* survivors_out, void* stream);

/* OBJECT-LEVEL render of NeRF_TP (evaluation, randomized=False): the two inside-sphere MLPs (slots 0, 1; slots 2, 3 are not
 * needed) are marched between a caller-given per-ray interval [near_obj, far_obj] (R floats each, device) - e.g. the output of
 * neo_aabb_multi for all boxes of a scene or for one of them - only for the rays that have one.  No background, no sphere
 * intersection and no sphere assertion.
 * HIT RULE: lo = max(near_obj, 1e-4) (the reference's near, neo360/model.py:277; also for an origin inside a box, where the
 * slab test gives tmin <= 0), hi = far_obj; a ray is a hit iff both bounds are finite and hi > lo.  The test is the negation of
 * the failing comparisons, so a NaN bound makes the ray a miss; the reference's "0 = no hit" sentinel falls out of the rule.
 * Hit rays, with the reference's own functions on the object interval: level 0 t = lo (1 - s) + hi s, s = linspace(0, 1,
 * n_coarse + 1) (helper.py:36-42); the evaluators of neo_tp_render with the quirk-Q1 direction index taken from the ray's own
 * index, R and `chunk` (a hit ray's result does not depend on which other rays hit); volumetric_rendering(in_sphere=True,
 * t_far=far_obj, white_bkgd) (helper.py:128-171): rgb (+ 1 - acc when white_bkgd: honoured here, unlike neo_tp_render), acc =
 * sum w, depth = sum w t; level 1 sample_pdf on the level-0 mids and weights[1:-1] with n_fine quantiles, sorted merge
 * (helper.py:218-231).  Missed rays, both levels: rgb = white_bkgd ? 1 : 0, acc = 0, depth = 0, tvals row = 0.
 * The hit rays are compacted in ascending ray order (deterministic, no atomics) and every kernel in between runs on compact rows.
 * hits_out [device, may be NULL]: receives the number of hit rays; the call never reads it on the host and synchronises nothing
 * (all launches are sized for R rays and take their row count from the device).  R == 0 zeroes hits_out and returns. */
typedef struct { float* rgb; float* acc; float* depth; float* tvals; } neo_tp_object_out;   /* any may be NULL; tvals (R, N_level) */
int neo_tp_render_objects(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs,
                          const float* near_obj, const float* far_obj, int R, int chunk, const float* src_poses, int NV,
                          float focal, float cx, float cy, int n_coarse, int n_fine, int white_bkgd,
                          const neo_tp_object_out* level0, const neo_tp_object_out* level1, int* hits_out, void* stream);

/* EVERY INSTANCE of a scene in one call: K per-instance intervals near_inst / far_inst (K,R floats each, device; e.g. the output of
 * neo_aabb_per_box), 0 <= K <= 32.  Pair (i, ray) is rendered exactly as neo_tp_render_objects renders `ray` between near_inst[i],
 * far_inst[i] - same evaluators, same quirk-Q1 direction index from the ray's own index, R and `chunk` - and the instances of a
 * ray are then composited in depth order.  No background, no sphere intersection and no sphere assertion.
 * HIT RULE (per pair, that of neo_tp_render_objects): lo = max(near_inst, 1e-4), hi = far_inst; a pair is a hit iff both bounds
 * are finite and hi > lo; the test is the negation of the failing comparisons, so a NaN bound makes the pair a miss.
 * The hit pairs are compacted in ascending (instance, ray) order (deterministic, no atomics; the count stays on the device) and
 * consumed in K WINDOWS of at most R rows: window p is rows [p R, p R + min(max(count - p R, 0), R)) of the pair list, one compact
 * launch chain of neo_tp_render_objects each (a compact launch holds at most R rows); an empty window's kernels leave at once.
 * PER-INSTANCE outputs rgb (K,R,3), acc (K,R), depth (K,R): row i is bitwise neo_tp_render_objects(near_inst[i], far_inst[i],
 * white_bkgd), missed pairs included (rgb = white_bkgd ? 1 : 0, acc = depth = 0).
 * COMPOSITE outputs comp_rgb (R,3), comp_acc (R), comp_depth (R), instance_id (R) int32: one thread per ray, plain fp32, in
 * exactly this order.  The ray's hit instances are taken in ascending lo, ties to the lower instance index; p_i = the instance's
 * premultiplied colour (its white_bkgd = 0 rgb), a_i = its acc, d_i = its depth.  COMPOSITE RECURRENCE: T = 1, rgb = depth = acc
 * = 0, best = 0, id = -1; for each instance in order: v = T * a_i; rgb += T * p_i; depth += T * d_i; acc += v; if v > best then
 * best = v, id = i; T = T * (1 - a_i).  Afterwards, if white_bkgd: rgb += 1 - acc.  A ray without hits gets rgb = white_bkgd ? 1 : 0,
 * acc = depth = 0, id = -1.  instance_id is the instance that contributes the largest visibility v to the ray (the counterpart
 * of the dataset's instance_mask).  Intervals of overlapping boxes are marched independently: density inside an overlap counts
 * twice.
 * Any output, and either level struct, may be NULL.  pairs_out [device, may be NULL]: receives the number of hit pairs; the call
 * never reads it on the host and synchronises nothing.  K == 0 writes the no-hit composite; R == 0 zeroes pairs_out and returns. */
typedef struct {
    float* rgb; float* acc; float* depth;                                  /* per instance: (K,R,3), (K,R), (K,R) */
    float* comp_rgb; float* comp_acc; float* comp_depth; int* instance_id; /* composite: (R,3), (R), (R), (R) */
} neo_tp_instance_out;
int neo_tp_render_instances(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs,
                            const float* near_inst, const float* far_inst, int K, int R, int chunk, const float* src_poses, int NV,
                            float focal, float cx, float cy, int n_coarse, int n_fine, int white_bkgd,
                            const neo_tp_instance_out* level0, const neo_tp_instance_out* level1, int* pairs_out, void* stream);

/* EDITED render: the scene WITHOUT an instance, or with an instance faded, tinted or - as a layer - standing somewhere else.
 * EDIT RULE (neo_tp_edit_rows; in place on rgbsigma (R,N,4) at the sample rows t (R,N)): near_inst / far_inst (K,R) [device],
 * 0 <= K <= 32, values of the ray parameter t of o + t rays_d exactly as neo_tp_render_objects reads them; pair (i, ray) is a hit by
 * the HIT RULE above (lo = max(near, 1e-4), hi = far, both finite, hi > lo; a NaN bound is a miss); sample j is INSIDE pair i iff
 * lo <= t_j && t_j <= hi (closed: neo_tp_render_objects places samples on both ends).  For i = 0 .. K-1 in index order, if inside:
 * sigma *= scale[i]; r *= tint[i][0]; g *= tint[i][1]; b *= tint[i][2] - plain fp32 multiplies, so overlapping intervals multiply;
 * a sample inside no interval is not written.  density_scale (K) and tint (K,3) are HOST arrays (NULL = all ones) that travel to
 * the kernel by value; they must be finite and >= 0.  K == 0 and R == 0 are valid calls.  Touches no context-owned memory. */
int neo_tp_edit_rows(neo_ctx* ctx, float* rgbsigma, const float* t, const float* near_inst, const float* far_inst, int K,
                     const float* density_scale, const float* tint, int R, int N, void* stream);

/* neo_composite mode 1 with 0 <= L <= 32 per-ray LAYERS spliced into the ray.  Layer l of a ray: key (L,R) a ray parameter, acc
 * (L,R) its opacity a_l, rgb (L,R,3) its premultiplied colour p_l, depth (L,R) its premultiplied depth d_l [all device].
 * LAYER RECURRENCE: a layer is valid iff key_l is finite and a_l > 0 (written so that a NaN is invalid); valid layers are ordered
 * by ascending key, ties to the lower index; keep_l = max(1 - a_l, 0) in fp32, then widened to double.  S(j) = the scene's own
 * exclusive transmittance before sample j (carry * excl of the fp64 scan of neo_composite), S_end the one after its last sample;
 * A(j) = the fp64 product, in layer order, of keep_l over the valid layers with key_l <= t_j; B(l) = that of the valid layers
 * ordered before l; j_l = the first sample with t_j >= key_l.  Sample j contributes with trans = (float)(S(j) A(j)), w' = alpha_j
 * trans: w' c_j to rgb, w' to acc, w' t_j to depth.  Layer l contributes with v = (float)(S(j_l) B(l)), or (float)(S_end B(l))
 * when no such sample exists: v p_l, v a_l, v d_l; visibility (L,R) receives v a_l, and 0 for an invalid layer.  lambda =
 * (float)(S_end * the product of all valid keeps).  weights (R,N) receives the SCENE weight alpha_j (float)S(j) - what neo_composite
 * writes, so that a resampling that follows does not depend on the layers.  A layer is a slab at its key, not a merged medium.
 * With no valid layer every output is bitwise neo_composite(mode 1, white_bkgd 0).  Any output may be NULL; R == 0 and L == 0 are
 * valid calls.  Touches no context-owned memory. */
typedef struct { const float* key; const float* rgb; const float* acc; const float* depth; } neo_tp_layers;
int neo_composite_layers(neo_ctx* ctx, const float* rgbsigma, const float* t, const float* rays_d, const float* t_far, int R, int N,
                         const neo_tp_layers* layers, int L, float* rgb, float* acc, float* depth, float* weights, float* lambda,
                         float* visibility /* (L,R) */, void* stream);

/* neo_tp_render (out_depth=True semantics, the coarse level always evaluated in full) with the EDIT RULE applied to the
 * inside-sphere rows of each level before their composite, and - when L > 0 - that composite done by the LAYER RECURRENCE with the
 * same layers at both levels.  The outside-sphere half, the resampling (on the scene weights), the merge, the flags and the scratch
 * lanes are neo_tp_render's.  With K == 0 (or every scale and tint 1) and L == 0 the twelve outputs are bitwise neo_tp_render's.
 * samples0 / samples1 (may be NULL, and any pointer in them): the level's sample rows fg_t, bg_s (R,N_level), its scene weights fg_w
 * (R,N_level) and - with layers - visibility (L,R). */
typedef struct { float* fg_t; float* fg_w; float* bg_s; float* visibility; } neo_tp_edit_samples;
int neo_tp_render_edited(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, const float* near_inst,
                         const float* far_inst, int K, const float* density_scale, const float* tint, const neo_tp_layers* layers,
                         int L, int R, int chunk, const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse,
                         int n_fine, const neo_tp_level_out* level0, const neo_tp_level_out* level1,
                         const neo_tp_edit_samples* samples0, const neo_tp_edit_samples* samples1, void* stream);

/* DECOMPOSED render: the frame split into per-instance layers that add up to it, a "rest" layer and an occlusion-aware id map.
 * DECOMPOSITION RULE (neo_tp_decompose_rows).  Per ray: the (N,4) rgb/sigma row c_j, the positions t_j, the scene weights w_j
 * exactly as neo_composite mode 1 writes them to `weights`, near_inst / far_inst (K,R) [device], 0 <= K <= 32, and optionally
 * bg_lambda (R).  Pair (i, ray) is a hit by the HIT RULE above (lo = max(near, 1e-4), hi = far, both finite, hi > lo; the negation
 * of the failing comparisons, so a NaN bound is a miss); sample j is INSIDE pair i iff lo <= t_j && t_j <= hi (closed, as in the
 * EDIT RULE).  owner(j) = the smallest hit i that j is inside of, else slot K, the REST: every sample has exactly one owner, and a
 * sample inside two boxes counts once.  For each slot s = 0 .. K: P_s = sum over owner(j) = s of w_j c_j (3 channels), a_s = sum
 * w_j, d_s = sum w_j t_j - plain fp32 in neo_composite's own order, slot by slot: lane j mod 64 of a 64-lane wave adds its samples
 * (the products w_j c_j, w_j t_j rounded first) in ascending j over the 64-sample rounds, starting from 0, then the butterfly of
 * the wave sum (offsets 32, 16, .. 1).  The order is part of the contract: a slot that owns every sample of a ray is bitwise
 * neo_composite's rgb / acc / depth on the same rows (adding 0.0f for another owner's sample changes nothing), a slot that owns
 * nothing is exactly 0.  No atomics; bitwise repeatable.
 * ID MAP id (R) int32: rest_total = a_K + bg_lambda (one fp32 add; a_K alone without bg_lambda); best = the largest a_i over i < K,
 * ties to the lower index; id = its index iff a_best > 0 && a_best >= rest_total, else -1.  A NaN mass never wins, and a NaN
 * rest_total gives -1.  The outside-sphere half of a ray always belongs to the rest: that is what bg_lambda stands for.
 * out: rgb (K+1,R,3), acc (K+1,R), depth (K+1,R), id (R); any pointer may be NULL.  1 <= N <= 1024.  K == 0 is a valid call (the
 * rest is then the whole ray), and so is R == 0.  Touches no context-owned memory. */
typedef struct { float* rgb; float* acc; float* depth; int* id; } neo_tp_decomposed_out;
int neo_tp_decompose_rows(neo_ctx* ctx, const float* rgbsigma, const float* t, const float* weights, const float* near_inst,
                          const float* far_inst, int K, int R, int N, const float* bg_lambda /* may be NULL */,
                          const neo_tp_decomposed_out* out, void* stream);

/* neo_tp_render (out_depth=True semantics, the coarse level always evaluated in full: the launch list of neo_tp_render_edited
 * without edits and layers, so the twelve outputs are bitwise neo_tp_render's) with the DECOMPOSITION RULE applied after the
 * inside-sphere composite of every level whose decomposed0 / decomposed1 is not NULL, on that level's rows, positions, scene
 * weights and bg_lambda.  The outside-sphere half, the resampling, the merge, the flags, the scratch lanes, the ray-grid hint, the
 * range guard and the sample-count limits are neo_tp_render's.  samples0 / samples1 (may be NULL, and any pointer in them): the
 * level's fg_t, bg_s and fg_w (R,N_level); `visibility` is not written. */
int neo_tp_render_decomposed(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, const float* near_inst,
                             const float* far_inst, int K, int R, int chunk, const float* src_poses, int NV, float focal, float cx,
                             float cy, int n_coarse, int n_fine, const neo_tp_level_out* level0, const neo_tp_level_out* level1,
                             const neo_tp_decomposed_out* decomposed0, const neo_tp_decomposed_out* decomposed1,
                             const neo_tp_edit_samples* samples0, const neo_tp_edit_samples* samples1, void* stream);

/* EMPTY-SPACE SKIPPING of the NeO-360 frame: a per-scene occupancy grid decides, sample by sample, which inside-sphere points the
 * evaluators see.
 * OCCUPANCY GRID.  G^3 cells over the world cube [-1, 1]^3; G = 8, 16 or a multiple of 32 in [32, 256].  On the device the grid is
 * G^3 / 32 words of 32 bits: cell (ix, iy, iz) is bit lin & 31 of word lin >> 5, lin = (ix G + iy) G + iz - the bits of a contiguous
 * bool (G,G,G) array in little-endian bit order.  The cell of a coordinate x, in fp32: i = min(max((int)floorf((x + 1.0f) *
 * (0.5f * G)), 0), G - 1).
 * KEEP RULE.  Sample j of ray r, at x = rays_o[r] + t[r][j] * rays_d[r] (one fp32 multiply and one fp32 add per coordinate, the
 * evaluators' own expression), is KEPT iff the bit of (cell(x_0), cell(x_1), cell(x_2)) is set, or a coordinate of x is not finite
 * (written as the negation of |x| < inf, so that a NaN survives to the caller), or there is no grid.
 *
 * neo_tp_set_occupancy copies `bits` [device, G^3 / 8 bytes] into context-owned memory; bits == NULL removes the grid.
 * neo_tp_set_scene removes it as well: a grid describes one scene (and its source poses and weights, which the library cannot
 * check).  neo_tp_set_skip_window: rays per window of neo_tp_render_skipping, 1 .. 65536, 0 = the default (4096); a window bounds
 * the extra workspace at (68 + 128) bytes per (ray, sample) of one window.  Results do not depend on it. */
int neo_tp_set_occupancy(neo_ctx* ctx, const uint32_t* bits, int G, void* stream);
int neo_tp_set_skip_window(neo_ctx* ctx, int rays);

/* The KEEP RULE on caller rows: rays_o, rays_d (R,3), t (R,N) -> keep (R,N) uint8 0 / 1.  bits [device] may be NULL (no grid: all
 * ones).  R == 0 is a valid call.  Touches no context-owned memory. */
int neo_tp_occupancy_keep(neo_ctx* ctx, const uint32_t* bits, int G, const float* rays_o, const float* rays_d, const float* t, int R,
                          int N, uint8_t* keep, void* stream);

/* A lattice of activated densities -> the bits of a grid.  sigma [device]: (M,M,M) floats, M = G probes, 1 <= probes <= 4; entry
 * (lx, ly, lz) belongs to cell (lx / probes, ly / probes, lz / probes).  A cell is raw-occupied iff one of its probes^3 entries is
 * not <= threshold (so a NaN entry is occupied and reaches the caller); occupied iff a cell at most `dilate` (0 .. 4) cells away in every axis is raw-occupied; and
 * cleared when none of its points lies inside the closed unit sphere: with h = G / 2 and n_a = i_a - h for i_a >= h, h - 1 - i_a
 * below, iff n_x^2 + n_y^2 + n_z^2 > h^2 (integers).  bits [device]: G^3 / 8 bytes.  Touches no context-owned memory. */
int neo_occupancy_from_sigma(neo_ctx* ctx, const float* sigma, int G, int probes, float threshold, int dilate, uint32_t* bits,
                             void* stream);

/* neo_tp_render (out_depth=True semantics, the coarse level always evaluated in full) in which an inside-sphere sample that the
 * KEEP RULE does not keep is NOT evaluated: its (rgb, sigma) row is (0, 0, 0, 0), which the composite turns into weight exactly 0.
 * Kept samples are evaluated by the evaluators' compact launches, one point per row, and are bitwise what neo_tp_render computes
 * for them; the composites, the level-1 resampling (on the resulting weights), the outside-sphere half (never skipped), the merge,
 * the flags, the scratch lanes and the ray-grid hint are neo_tp_render's.  With every cell set, or no grid installed, the twelve
 * outputs are bitwise neo_tp_render's; with no cell set fg_rgb = fg_acc = 0, bg_lambda = 1 and no inside-sphere point is evaluated.
 * samples0 / samples1 (may be NULL, and any pointer in them): the level's fg_t, fg_w, bg_s (R,N_level), its keep mask fg_keep
 * (R,N_level) uint8 and its inside-sphere rows fg_rows (R,N_level,4).  kept (may be NULL): int64[2] on the device, the kept
 * samples of level 0 and level 1; nothing is read back. */
typedef struct { float* fg_t; float* fg_w; float* bg_s; uint8_t* fg_keep; float* fg_rows; } neo_tp_skip_samples;
int neo_tp_render_skipping(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                           const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse, int n_fine,
                           const neo_tp_level_out* level0, const neo_tp_level_out* level1, const neo_tp_skip_samples* samples0,
                           const neo_tp_skip_samples* samples1, long long* kept, void* stream);

/* EARLY RAY TERMINATION of the NeO-360 frame: a ray's inside-sphere march stops once its transmittance has fallen below eps, and
 * the outside-sphere half is not evaluated for rays that are opaque at both levels.  No per-scene artefact, no trained threshold.
 * STOP RULE.  A level's N inside-sphere samples are cut into SEGMENTS of `segment` samples, `segment` a positive multiple of 64; the
 * last segment may be shorter.  64 because the inside-sphere composite (neo_composite mode 1) scans its transmittance product in
 * rounds of 64 samples and carries an fp64 product `carry` between rounds: the transmittance it assigns to the first sample of a
 * round is exactly (float)carry.  At a boundary b that is a multiple of 64, "the transmittance in front of sample b" is therefore a
 * quantity the composite itself defines, bit for bit; it depends only on rows [0, b) and on t[b].  The march forms carry with the
 * composite's own expressions - alpha = alpha(sigma * (delta * |d|)), keep = (1 - alpha) + 1e-10f, the 64-lane inclusive product scan
 * in fp64, carry *= the round's last lane - so its value IS the composite's.
 * Segment 0 is always evaluated.  Segment k >= 1 of a ray is evaluated iff every earlier boundary b satisfied !((float)carry_b < eps)
 * - a negation, so a NaN keeps marching (as in the culled call).  stop[r] = the number of leading samples evaluated: N or a segment
 * boundary.  A sample at or behind stop is NOT evaluated and its (rgb, sigma) row is (0, 0, 0, 0); the composite gives it weight
 * exactly 0 and leaves the product unchanged (1.0f + 1e-10f == 1.0f).  The evaluated samples are a prefix, so their weights are
 * bitwise neo_tp_render's, and a stopped ray's bg_lambda is the transmittance at stop (< eps).
 * LEVELS.  Level 1 follows the rule.  Level 0 follows it only with coarse != 0; otherwise its inside-sphere launch is the plain dense
 * one (ray-patch order, density-only when no level-0 colour or depth is asked for).  coarse != 0 changes the level-0 weights behind
 * the stop from "less than eps in total" to 0, so the level-1 positions move: NO bound is claimed for that mode.
 * BACKGROUND.  The launch order is neo_tp_render_culled's: the foreground of both levels first; a ray's two outside-sphere
 * evaluations run iff !(bg_lambda_0 < eps) || !(bg_lambda_1 < eps) on the returned lambdas; the survivors go through that call's
 * compact path; a culled ray gets rgb = fg_rgb, bg_rgb = 0, depth = fg_depth.
 * eps in [0, 1).  eps == 0 stops and culls nothing: all twelve outputs are bitwise neo_tp_render's.  A ray that never stops and is
 * not culled is bitwise neo_tp_render's at any eps.
 * BOUND (coarse == 0, level 1; L = the returned bg_lambda < eps of a stopped ray, F = the plain frame's bg_lambda <= L).  With
 * T_{i+1} = T_i (1 - alpha_i + 1e-10), a weight is w_i = alpha_i T_i = T_i - T_{i+1} + 1e-10 T_i, so the skipped weights sum to
 * S = L - F + 1e-10 sum T_i <= (L - F) + 1024e-10 L.  Colours lie in (-0.001, 1.001); the background colour B is a sum of weights
 * (<= 1 + 1e-7) times such colours.  A surviving ray changes by (L - F) B - sum_skipped w_i c_i, a sum of S-weighted differences
 * B - c_i with |B - c_i| < 1.002 (1 + 1e-7); a culled ray by -sum_skipped w_i c_i - F B, at most 1.001 (1 + 1e-7) (S + F).  Either
 * way |rgb change| < 1.0021 L per channel in real arithmetic; the constant 1.003 leaves 0.0009 L for the fp32 rounding of the two
 * sums being compared (about 1e-7), which covers it wherever L > 2e-4 - below that the change is at the plain frame's own rounding.
 * Depth: inside positions are <= t_far, the background depth is a sum of weights times inverse radii in [0, 1], and the two terms of
 * the change have opposite signs (survivor) or sum to <= t_far (L - F) + F (culled): |depth change| <= max(t_far, 1) (1 + 1e-7) L,
 * which is below the (t_far + 1.001) L the tests assert.
 * Sphere-miss assertions cover every ray.  A sample that is not evaluated takes no part in the fp16 range check.  white_bkgd does
 * not exist here (ignored by neo_tp_render).  No call synchronises the device.  An installed occupancy grid is not read; the
 * ray-grid hint is taken by a dense level-0 launch only (compact launches never take it).
 * Windows: a point list (one segment of the alive rays of one window) has at most
 * skip_window x N_level rows - neo_tp_set_skip_window's bound and workspace - so a window holds skip_window N_level / segment rays;
 * results do not depend on it.
 * samples0 / samples1 (may be NULL, and any pointer in them): the level's fg_t, fg_w, bg_s (R,N_level; level-1 bg_s rows of culled
 * rays are zero), stop (R) int32 and its inside-sphere rows fg_rows (R,N_level,4).  kept (may be NULL): int64[2] on the device, the
 * evaluated inside-sphere samples per level (= sum of stop).  survivors_out (may be NULL): int on the device, the rays whose
 * background ran. */
typedef struct { float* fg_t; float* fg_w; float* bg_s; int* stop; float* fg_rows; } neo_tp_term_samples;
int neo_tp_render_terminating(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                              const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse, int n_fine,
                              const neo_tp_level_out* level0, const neo_tp_level_out* level1, float eps, int segment, int coarse,
                              const neo_tp_term_samples* samples0, const neo_tp_term_samples* samples1, long long* kept,
                              int* survivors_out, void* stream);

/* ACCELERATED FRAME: neo_tp_render_terminating that also obeys the installed occupancy grid - the KEEP RULE and the STOP RULE together.
 * LEVEL 1, AND LEVEL 0 WITH coarse != 0.  Sample j of ray r is evaluated iff it satisfies the KEEP RULE of the installed grid AND
 * j < stop[r].  stop is the STOP RULE applied to the level's rows in which the samples that are not kept are (0, 0, 0, 0): a zero row
 * leaves the composite's fp64 carry alone (1.0f + 1e-10f == 1.0f), so stop is neo_tp_termination_stops on the masked rows, bit for
 * bit.  Segment 0 is always marched (its kept samples evaluated), `segment` is a positive multiple of 64, a NaN transmittance marches
 * on.  A sample that is not evaluated has a zero row and weight exactly 0; an evaluated one is bitwise neo_tp_render's for its
 * position.
 * LEVEL 0 WITH coarse == 0 obeys the grid only, exactly as level 0 of neo_tp_render_skipping (stop = N_0).
 * BACKGROUND AND LAUNCH ORDER are neo_tp_render_terminating's: the foreground of both levels first; a ray's two outside-sphere
 * evaluations run iff !(bg_lambda_0 < eps) || !(bg_lambda_1 < eps), through the same compact path; a culled ray gets rgb = fg_rgb,
 * bg_rgb = 0, depth = fg_depth.
 * NO GRID INSTALLED: the KEEP RULE keeps everything and every output is bitwise neo_tp_render_terminating's (level 0 without
 * `coarse` is then that call's plain dense launch in ray-patch order).  eps == 0: every output is bitwise neo_tp_render_skipping's
 * with the same grid.  Both: bitwise neo_tp_render.
 * BOUND (coarse == 0, level 1), against neo_tp_render_skipping with the same grid: level 0, and therefore the level-1 positions and
 * the keep masks, are identical in the two calls, and the argument of the BOUND above only uses that the rows behind the stop
 * become zero - it holds with "the plain frame" read as the skipping frame: |rgb change| <= 1.003 bg_lambda per channel and
 * |depth change| <= (t_far + 1.001) bg_lambda, with the returned bg_lambda < eps of a stopped ray.  Nothing is claimed for coarse != 0,
 * and nothing against neo_tp_render (that is the grid's own error, which the library cannot bound).
 * Windows and workspace: the terminating frame's, plus one byte per candidate of a segment launch and one int per 1024 of them; a
 * point list still has at most skip_window x N_level rows.  neo_tp_set_scene drops the grid: the next call is the terminating frame.
 * No call synchronises the device.
 * samples0 / samples1 (may be NULL, and any pointer in them): as neo_tp_term_samples, plus fg_keep (R,N_level) uint8, the KEEP RULE
 * on the WHOLE row, samples behind the stop included (all ones without a grid): the evaluated set is fg_keep & (j < stop).
 * kept: int64[2], the evaluated inside-sphere samples per level.  survivors_out: the rays whose background ran. */
typedef struct { float* fg_t; float* fg_w; float* bg_s; int* stop; uint8_t* fg_keep; float* fg_rows; } neo_tp_accel_samples;
int neo_tp_render_accelerated(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                              const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse, int n_fine,
                              const neo_tp_level_out* level0, const neo_tp_level_out* level1, float eps, int segment, int coarse,
                              const neo_tp_accel_samples* samples0, const neo_tp_accel_samples* samples1, long long* kept,
                              int* survivors_out, void* stream);

/* The STOP RULE on caller rows: rgbsigma (R,N,4), t (R,N), rays_d (R,3), t_far (R) -> stop (R) int32, the samples a march over
 * these rows evaluates, and trans (R), the fp32 transmittance at the stop ((float)carry there; bg_lambda of the composite when
 * stop == N).  The kernel is the frame's.  R == 0 is a valid call.  Touches no context-owned memory. */
int neo_tp_termination_stops(neo_ctx* ctx, const float* rgbsigma, const float* t, const float* rays_d, const float* t_far, int R, int N,
                             float eps, int segment, int* stop, float* trans, void* stream);

/* MARCHING FRAME: the one driver behind neo_tp_render_terminating (use_grid == 0) and neo_tp_render_accelerated (use_grid != 0), with
 * one more switch: outside != 0 carries the early termination through the OUTSIDE-sphere march of the rays whose background runs.
 * OUTSIDE STOP RULE.  For a ray r whose background runs - a survivor of the cull !(bg_lambda_0 < eps) || !(bg_lambda_1 < eps), which
 * stays exactly as it is - a level's N outside-sphere samples are cut into SEGMENTS of `segment` samples, `segment` the call's value,
 * a positive multiple of 64; the last segment may be shorter.  The samples are s = 1/r DESCENDING, as neo_composite mode 2 reads
 * them.  carry_b is mode 2's fp64 product in front of sample b, formed with its own lines: delta_i = s_i - s_{i+1}, the last one
 * 1e10, no |d| factor, keep = (1 - alpha(sigma * delta)) + 1e-10f, the 64-lane inclusive product scan in fp64, carry *= the round's
 * last lane.  The RUNNING VALUE at a boundary b (a multiple of `segment`) is v_b = bg_lambda_level[r] * (float)carry_b: one fp32
 * multiply of the level's RETURNED lambda with the background transmittance that the composite assigns to sample b, bit for bit.  It
 * is the factor with which everything at or behind b reaches the pixel.  Segment 0 always runs.  Segment k >= 1 runs iff every
 * earlier boundary b satisfied !(v_b < eps) - a negation, so a NaN keeps marching.  bg_stop[r] = the leading samples evaluated: N or
 * a boundary; 0 for a culled ray.  bg_value[r] = v at the stop (with bg_stop == N: bg_lambda * (float)(the product over all N
 * samples)); 0 for a culled ray.  A row at or behind the stop is NOT evaluated and is (0, 0, 0, 0); mode 2 gives it weight exactly 0
 * and leaves the product unchanged, because alpha(0 * delta) = 0 - also for the last delta 1e10 - and 1.0f + 1e-10f == 1.0f.  The
 * evaluated samples are a prefix, so their weights are bitwise those of the call with outside == 0.
 * LEVELS.  Level 1 follows the rule.  Level 0 follows it only with coarse != 0: its weights feed the level-1 outside resampling, so
 * stopping it moves positions, and NO bound is claimed for that mode (as for the inside `coarse`).  A level that does not follow the
 * rule is the compact launch of neo_tp_render_culled: bg_stop = N for a survivor.
 * eps == 0 stops nothing (v >= 0 or NaN): all twelve outputs are bitwise neo_tp_render's.  outside == 0: every output is bitwise
 * neo_tp_render_accelerated's (use_grid != 0) or neo_tp_render_terminating's (use_grid == 0), launch for launch.
 * BOUND (coarse == 0, level 1), against the SAME call with outside == 0.  The foreground of both levels runs first and reads nothing
 * of the background: fg_rgb, fg_acc, bg_lambda, the inside stop and the cull set are bitwise equal in the two calls; so are the
 * level-0 outside weights and therefore the level-1 outside positions.  Let a ray's level-1 outside march stop at b, lam = its
 * bg_lambda_1, T_b = carry_b.  With T_{i+1} = T_i (1 - alpha_i + 1e-10), a weight is w_i = alpha_i T_i = T_i - T_{i+1} + 1e-10 T_i,
 * so the skipped weights sum to at most T_b (1 + N 1e-10).  Colours lie in (-0.001, 1.001); s in [0, 1].  v_b carries two fp32
 * roundings (the conversion of carry_b and the multiply), so lam T_b <= v_b (1 + 2^-24)^2 < eps (1 + 2^-23) for normal v_b.  Hence
 * |rgb change| = lam |sum_skipped w_i c_i| < 1.001 (1 + N 1e-10)(1 + 2^-23) eps < 1.0011 eps per channel and |depth change| <=
 * lam sum_skipped w_i s_i < 1.0000002 eps in real arithmetic.  The tests assert 1.003 eps for both: the margin 0.0019 eps covers
 * the fp32 rounding of the two sums being compared (about 3e-7 lam) wherever eps > 2e-4 lam, as in the BOUND of the inside rule.
 * A ray whose outside march never stops is bitwise the ray of the call with outside == 0.
 * On the device the march runs on the COMPACT background rows of the culled frame (row k belongs to the k-th survivor; the count is
 * a device word): per window and segment the alive rows are compacted on the running value, their samples of the segment go
 * through the outside evaluator's compact launch as single points carrying the ray's origin, direction and far, and scatter into
 * zero-filled rows.  Windows: skip_window x N_level / segment rows, as for the inside march; results do not depend on them.  The
 * composites, the resampling, the merges, the flags and the lanes are the culled frame's.  No call synchronises the device.
 * samples0 / samples1 (may be NULL, and any pointer in them): neo_tp_accel_samples' fields, then bg_stop (R) int32, bg_value (R) and
 * bg_rows (R,N_level,4), the level's outside-sphere rows dense by ray (zero rows for culled rays and behind bg_stop).  kept (may be
 * NULL): int64[4] on the device, the evaluated samples inside the sphere per level, then outside the sphere per level (= the sums of
 * stop and of bg_stop).  survivors_out: the rays whose background ran. */
typedef struct {
    float* fg_t; float* fg_w; float* bg_s; int* stop; uint8_t* fg_keep; float* fg_rows;
    int* bg_stop; float* bg_value; float* bg_rows;
} neo_tp_march_samples;
int neo_tp_render_marching(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                           const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse, int n_fine,
                           const neo_tp_level_out* level0, const neo_tp_level_out* level1, float eps, int segment, int coarse,
                           int use_grid, int outside, const neo_tp_march_samples* samples0, const neo_tp_march_samples* samples1,
                           long long* kept, int* survivors_out, void* stream);

/* The OUTSIDE STOP RULE on caller rows: rgbsigma (R,N,4), s (R,N) descending, bg_lambda (R) -> stop (R) int32, the samples a march
 * over these rows evaluates (every row is treated as a ray whose background runs), and value (R), the running value at the stop.
 * The kernel is the frame's.  R == 0 is a valid call.  Touches no context-owned memory. */
int neo_tp_termination_stops_outside(neo_ctx* ctx, const float* rgbsigma, const float* s, const float* bg_lambda, int R, int N,
                                     float eps, int segment, int* stop, float* value, void* stream);

/* ---- scene encoder: pillar stage -------------------------------------------------------- */
/* Weights of the pillar stage of GridEncoder (models/neo360/encoder_tp_fusion_conv.py:263-279, :364-373).
 * weights/biases [host arrays of 9 device pointers], order: depth_fc.common_branch.0 (512x518), depth_fc.common_branch.2,
 * depth_fc.depth_encoder, pillar_aggregator_xz.0 (512x513), pillar_aggregator_xz.2 (1x512), pillar_aggregator_yz.0, .2,
 * pillar_aggregator_xy.0, .2.  Packs the fragments of both arithmetics (split fp16, and about 6 MB of fp32 fragments for
 * the exact kernels), so neo_ctx_set_precision may change between calls without another upload. */
int neo_enc_upload(neo_ctx* ctx, const float* const* weights, const float* const* biases, void* stream);

/* GridEncoder.forward from the world grid to the inputs of its floor-plan conv nets (:472-578): for every cell of the
 * G0 x G1 x G2 world grid (x, y in [-1,1], z in [0,1]) and source view, [pixel-aligned latent | camera xyz | masked
 * direction] -> depth_fc -> three axis scorers -> softmax along x / y / z -> weighted sums.  latent (NV,512,Hf,Wf) NCHW =
 * SpatialEncoder's output; src_poses [host] NV*16; focal / cx / cy = view 0's intrinsics (:491-493).  Outputs
 * channels-last: fp_yz (NV,G1,G2,512), fp_xz (NV,G0,G2,512), fp_xy (NV,G0,G1,512) (the reference permutes them to NCHW
 * for its conv nets, :580-592).  Runs in the context's arithmetic (neo_ctx_set_precision): mode 1 = fp16 MFMA on hi/lo-split
 * operands behind the range guard (a latent texel or a weight at or beyond 65504, a latent whose largest |x| or a layer
 * whose largest |w| is non-zero and below 2^-6 raises flag bit 1; bit 2 as well when it is a weight); mode 0 = exact fp32 MFMA, no range check, no flag bit - what a caller whose guard tripped runs again. */
int neo_enc_floorplans(neo_ctx* ctx, const float* latent, int NV, int Hf, int Wf, float image_w, float image_h,
                       const float* src_poses, float focal, float cx, float cy, int G0, int G1, int G2,
                       float* fp_yz, float* fp_xz, float* fp_xy, void* stream);

/* The pillar stage under autograd (GridEncoder trained as the reference trains it, models/neo360/model.py:697-820).
 * neo_enc_floorplans_train: neo_enc_floorplans with the activations the backward needs written to `tape`, a CALLER-owned
 * device buffer of neo_enc_train_tape_floats(NV, G0, G1, G2) floats = h1, h2, L (M x 512 each, M = NV G0 G1 G2 cell-views)
 * and the three score vectors (xz, yz, xy); same kernels, same arithmetic (either mode), same range guard and flags: the
 * floor-plans are bitwise those of neo_enc_floorplans in the same mode, and the tape layout does not depend on the mode.
 * At most 8,388,480 cell-views per call.
 * neo_enc_floorplans_backward: exact fp32 MFMA.  w / b: the nine layers as fp32 device tensors in neo_enc_upload's order;
 * latent / geometry: the forward's arguments; tape: the forward's, only read (a second backward of the same tape gives the
 * same gradients); g_yz / g_xz / g_xy: gradients of the floor-plans, channels-last like the outputs; gw / gb [host arrays of
 * 9 device pointers]: accumulated into (zeroed by the caller; the parameter gradients are reduced in a fixed order and
 * repeat bitwise); g_latent (NV,512,Hf,Wf) NCHW: accumulated (atomically: repeats to rounding), may be NULL.  No gradient
 * reaches src_poses, focal or the principal point.  The first layer's input is re-gathered from the latent, not taped; the
 * scratch (about 3 M x 512 floats + the channels-last latent gradient) is context-owned. */
long neo_enc_train_tape_floats(int NV, int G0, int G1, int G2);
int neo_enc_floorplans_train(neo_ctx* ctx, const float* latent, int NV, int Hf, int Wf, float image_w, float image_h,
                             const float* src_poses, float focal, float cx, float cy, int G0, int G1, int G2, float* tape,
                             float* fp_yz, float* fp_xz, float* fp_xy, void* stream);
int neo_enc_floorplans_backward(neo_ctx* ctx, const float* const* w, const float* const* b, const float* latent, int NV, int Hf,
                                int Wf, float image_w, float image_h, const float* src_poses, float focal, float cx, float cy,
                                int G0, int G1, int G2, const float* tape, const float* g_yz, const float* g_xz, const float* g_xy,
                                float* const* gw, float* const* gb, float* g_latent, void* stream);

/* ---- training-side operators ----------------------------------------------------------- */
/* Counter-based uniforms in [0,1): out[r][c] = (Philox4x32-10(key = seed, counter = (r, c, stream_id, 0))[0] >> 8) 2^-24
 * - the generator behind every randomized=True sampler here (the reference draws torch.rand: helper.py:49, :196). */
/* dst[b][c][r] = src[b][r][c]: batched 2-D transpose (fp32, tiled through LDS, out of place).  NCHW <-> channels-last of a feature map
 * under autograd: (NV, C, H W) -> (NV, H W, C) is batch NV, rows C, cols H W; the gradient goes back with rows H W, cols C
 * (the reference keeps NCHW and permutes inside grid_sample: encoder_tp_fusion_conv.py:180-206). */
int neo_transpose(neo_ctx* ctx, const float* src, long batch, int rows, int cols, float* dst, void* stream);
int neo_rand_uniform(neo_ctx* ctx, uint64_t seed, uint32_t stream_id, int rows, int cols, float* out, void* stream);

/* neo360/helper.py:24-75 sample_along_rays for both regions: far (R) from neo_intersect_sphere, near = 1e-4.
 * u_fg / u_bg (R, n_coarse+1) uniforms = randomized=True (stratified jitter, :44-51); both NULL = randomized=False.
 * fg_t (R, n_coarse+1) ascending t; bg_s (R, n_coarse+1) descending inverse radius. */
int neo_tp_sample_level0(neo_ctx* ctx, const float* far, int R, int n_coarse, const float* u_fg, const float* u_bg,
                         float* fg_t, float* bg_s, void* stream);

/* neo_resample with one row of quantiles per ray, u (R, n_new) in [0,1): sorted_piecewise_constant_pdf with
 * randomized=True (neo360/helper.py:195-196; the draws need not be sorted). */
int neo_resample_u(neo_ctx* ctx, const float* t_prev, const float* weights, const float* u, int R, int n_prev,
                   int n_new, int descending, float* t_out, void* stream);

/* Backward of neo_composite (same mode / inputs): upstream gradients g_rgb (R,3), g_acc (R), g_depth (R),
 * g_weights (R,N), g_lambda (R) (any may be NULL = zero) -> g_rgbsigma (R,N,4) = dL/d(rgb, sigma) per sample.
 * The sample positions carry no gradient (the reference detaches them, helper.py:224). */
int neo_composite_backward(neo_ctx* ctx, int mode, const float* rgbsigma, const float* t, const float* rays_d,
                           const float* t_far, int R, int N, int white_bkgd, const float* g_rgb,
                           const float* g_acc, const float* g_depth, const float* g_weights,
                           const float* g_lambda, float* g_rgbsigma, void* stream);

/* torch_efficient_distloss.eff_distloss(w, m, interval) (requirements.txt:29; call site neo360/model.py:1246-1260):
 * per ray interval/3 sum w^2 + 2 sum_{i>j} w_i w_j (m_i - m_j) evaluated with prefix sums.  loss_rays (R) = per-ray
 * loss (the reference returns their mean), grad_w (R,N) = d loss_ray / d w; either may be NULL. */
int neo_distloss(neo_ctx* ctx, const float* w, const float* m, int R, int N, float interval, float* loss_rays,
                 float* grad_w, void* stream);

/* NeRFPPMLP for TRAINING (the module the reference's training step differentiates, neo360/model.py:110-158 under
 * :697-820) on the rows the reference forms: [pos_enc | local 512 | world 128] per point-view, given as the three dense
 * tensors they are concatenated from (x_enc (NV*P, 21 input_ch), local_feat (NV*P, 512), world_feat (NV*P, 128): the
 * concatenation, 3.3 GB for a reference chunk level, is never materialised), and cond (NV*P, 27) = view-direction
 * encodings; view-major rows (row = v P + p).  w / b [host]: nine DEVICE
 * pointers each, order and nn.Linear (out, in) layout of neo_tp_upload_mlp (pts_linears.0..3, views_linear.0, .1,
 * bottleneck, density, rgb).  forward: raw_rgb (P,3), raw_sigma (P,1) (pre-activation, as the module returns them); the
 * activations the backward needs are written to `tape`, a CALLER-owned device buffer of neo_tp_mlp_train_tape_floats(NV, P)
 * floats (a training step runs the four MLPs of both levels forward before the first backward: one tape per call).
 * backward (with the tape, inputs, cond and weights of that forward; g_* = upstream gradients):
 * gw / gb [host]: nine device pointers each to gradient buffers of the weights' / biases' shapes, ZEROED by the caller
 * (partial sums are accumulated atomically); g_x_enc / g_local / g_world = gradients of the three input tensors
 * (overwritten; each may be NULL) - the latter two feed neo_tp_gather_backward.  Exact fp32 arithmetic (v_mfma_f32_32x32x2_f32).  At most
 * 4.19 M rows per call. */
long neo_tp_mlp_train_tape_floats(int NV, long P);
int neo_tp_mlp_train_forward(neo_ctx* ctx, int input_ch, const float* const* w, const float* const* b, const float* x_enc,
                             const float* local_feat, const float* world_feat, const float* cond, int NV, long P, float* tape,
                             float* raw_rgb, float* raw_sigma, void* stream);
int neo_tp_mlp_train_backward(neo_ctx* ctx, int input_ch, const float* const* w, const float* x_enc, const float* local_feat,
                              const float* world_feat, const float* cond, int NV, long P, const float* tape,
                              const float* g_rgb, const float* g_sigma, float* const* gw, float* const* gb, float* g_x_enc,
                              float* g_local, float* g_world, void* stream);

/* The vanilla NeRFMLP for training (vanilla_nerf/model.py:100-125 under the training step :255-283), same contract:
 * x0 (R, 63) encoded points, cond (R, 27) = each row's view-direction encoding (the ray's, tiled over its samples);
 * w / b [host]: twelve device pointers each in the order of neo_vanilla_upload_mlp; tape: caller-owned,
 * neo_vanilla_mlp_train_tape_floats(R) floats; backward: gw / gb zeroed by the caller, g_x0 (R, 63) / g_cond (R, 27) may
 * be NULL.  Exact fp32 arithmetic. */
long neo_vanilla_mlp_train_tape_floats(long R);
int neo_vanilla_mlp_train_forward(neo_ctx* ctx, const float* const* w, const float* const* b, const float* x0, const float* cond,
                                  long R, float* tape, float* raw_rgb, float* raw_sigma, void* stream);
int neo_vanilla_mlp_train_backward(neo_ctx* ctx, const float* const* w, const float* x0, const float* cond, long R,
                                   const float* tape, const float* g_rgb, const float* g_sigma, float* const* gw,
                                   float* const* gb, float* g_x0, float* g_cond, void* stream);

/* Sample points of the training call and their encodings (round 5; replaces torch restatements of neo360/helper.py:24-75,
 * :401-451, util.py:52-70 in the host code): for the samples tvals (R,N) of one region - input_ch 3: inside the sphere, t along
 * the ray; 4: outside, descending inverse radius s, `far` (R) required - look (R*N,3) = the world points the features are looked up
 * at (inside o + t d; outside o + (far (1-s) + 3 s) d), x_enc (NV, R*N, 21*input_ch) = pos_enc (reference feature order,
 * helper.py:121-125) of the camera-frame point per source view (outside: [R_v x' + t_v | s], x' the inverted-sphere point).
 * The device code is the evaluators' own per-point set-up: both paths see bitwise the same points. */
int neo_tp_train_points(neo_ctx* ctx, int input_ch, const float* rays_o, const float* rays_d, const float* tvals, const float* far,
                        int R, int N, const float* src_poses, int NV, float* look, float* x_enc, void* stream);
/* The reference's output activations (neo360/model.py:380-385) as one op: rgbsigma (P,4) = (sigmoid(raw_rgb) 1.002 - 0.001,
 * softplus(raw_sigma + noise * noise_scale - 1)); noise (P) may be NULL (model.py:381-384: density_noise).  backward: gradients
 * of raw_rgb (P,3) and raw_sigma (P) from g_rgbsigma (P,4). */
int neo_tp_activate(neo_ctx* ctx, const float* raw_rgb, const float* raw_sigma, const float* noise, float noise_scale, long P,
                    float* rgbsigma, void* stream);
int neo_tp_activate_backward(neo_ctx* ctx, const float* raw_rgb, const float* raw_sigma, const float* noise, float noise_scale, long P,
                             const float* g_rgbsigma, float* g_rgb, float* g_sigma, void* stream);

/* Projected-space training (round 5): the training analogue of the evaluators' pre-projection.  NeRFPPMLP reads the 512-channel
 * latent only through W0_loc and the skip half W3_loc (neo360/model.py:123-137), and bilinear interpolation is linear, so the caller
 * forms G = latent . [W0_loc | W3_loc]^T per TEXEL (a plain (texels, 512) x (512, 256) GEMM under autograd), gathers 256 instead of
 * 512 channels and hands them to the MLP as `pre` (NV*P, 256) = the local features' contribution to the pre-activations of layer 0
 * and of the skip half of layer 3.  neo_tp_gather_map / _backward: the lookup (and its scatter-add backward) in a CALLER-OWNED
 * channels-last map (NV Hf Wf, C), C % 64 == 0, at get_local_feats' taps of the scene geometry set with neo_tp_set_scene;
 * `texels` = rows of the caller's map (and of g_map): it MUST equal NV Hf Wf of the uploaded geometry, anything else is rejected
 * (the kernels index the map from the context's geometry - a map of another resolution would be read and scattered out of bounds).
 * neo_tp_mlp_train_forward_pre / _backward_pre: as neo_tp_mlp_train_forward / _backward with `pre` in place of the local feature
 * rows; the backward returns g_pre (NV*P, 256) = [dL/dz0 | dL/dz3] and leaves the local columns of gw[0] / gw[3] untouched (their
 * gradient is formed in texel space by the caller's GEMM). */
int neo_tp_gather_map(neo_ctx* ctx, const float* map, long texels, int C, const float* pts, long P, const float* src_poses, int NV, float focal,
                      float cx, float cy, float* out, void* stream);
int neo_tp_gather_map_backward(neo_ctx* ctx, long texels, int C, const float* pts, long P, const float* src_poses, int NV, float focal, float cx,
                               float cy, const float* g_out, float* g_map, void* stream);
/* The same lookup in a C-column SLICE of a wider channels-last map (round 6): row pitch `pitch` floats, `map` / `g_map` point at the
 * slice's first column (16-byte aligned).  One merged texel-space projection (texels, 4 x 256) then serves the four MLPs of NeRF_TP:
 * each gathers - and scatters its gradient into - its own 256 columns of ONE map / ONE gradient buffer. */
int neo_tp_gather_map_slice(neo_ctx* ctx, const float* map, long texels, long pitch, int C, const float* pts, long P, const float* src_poses,
                            int NV, float focal, float cx, float cy, float* out, void* stream);
int neo_tp_gather_map_slice_backward(neo_ctx* ctx, long texels, long pitch, int C, const float* pts, long P, const float* src_poses, int NV,
                                     float focal, float cx, float cy, const float* g_out, float* g_map, void* stream);
int neo_tp_mlp_train_forward_pre(neo_ctx* ctx, int input_ch, const float* const* w, const float* const* b, const float* x_enc,
                                 const float* pre, const float* world_feat, const float* cond, int NV, long P, float* tape,
                                 float* raw_rgb, float* raw_sigma, int* chain_mode, void* stream);
int neo_tp_mlp_train_backward_pre(neo_ctx* ctx, int input_ch, const float* const* w, const float* x_enc, const float* world_feat,
                                  const float* cond, int NV, long P, const float* tape, const float* g_rgb, const float* g_sigma,
                                  float* const* gw, float* const* gb, float* g_x_enc, float* g_pre, float* g_world, int chain_mode,
                                  void* stream);

/* One linear layer of a training chain the caller composes (models whose MLP has no fused training kernel: PixelNeRF's decoder,
 * vanilla_nerf/model_pixel.py:96-131): y (rows, out_f) = x (rows, in_f) W^T + bias [then ReLU] (accumulate != 0: added onto y
 * first), and the input gradient gx (rows, in_f) (+)= gy (rows, out_f) W.  W (out_f, in_f) with row pitch ldw (a column block of
 * a wider matrix is addressed by its pitch), fp32, exact fp32 MFMA.  With neo_linear_weight_grad these are torch's addmm and its
 * two backward products. */
int neo_linear_forward(neo_ctx* ctx, long rows, int out_f, int in_f, const float* x, long ldx, const float* w, long ldw,
                       const float* bias, int relu, int accumulate, float* y, long ldy, void* stream);
int neo_linear_input_grad(neo_ctx* ctx, long rows, int in_f, int out_f, const float* gy, long ldy, const float* w, long ldw,
                          int accumulate, float* gx, long ldx, void* stream);
/* Schedule of the projected-space training chains (neo_tp_mlp_train_forward_pre, neo_pix_mlp_train_forward_pre), process-wide: 1 (default) =
 * everything per row - layers 0..3, bottleneck, view layer 0; backward: the input-gradient chain g_y0 -> g_z0 and g_world - as ONE
 * kernel each way with the activation tile in LDS and every layer written to HBM once (csrc/train_chain.h); 0 = one GEMM launch per
 * layer (rounds 3-5).  Same exact-fp32 products in both; mode < 0 only queries.  Returns the previous mode.
 * The mode applies to the NEXT forward: the two modes write different tape layouts, so each *_forward_pre reports the mode it used
 * through `chain_mode` (may be null) and the matching *_backward_pre must be passed that value - the backward never reads this
 * setting, and changing it between a forward and its backward is harmless. */
int neo_train_chain_mode(int mode);
/* PixelNeRF's late-fusion MLP under autograd as ONE chain each way (round 6; vanilla_nerf/model_pixel.py:96-131 inside the training
 * step :255-300): rows R = NV * P view-major; x_enc (R, 63) camera-frame encodings, pre (R, 128) = the gathered PROJECTED latent
 * W0[:, 63:575] f (the 512-wide product is formed per texel by the caller, as for NeRFPPMLP), cond (R, 27) direction encodings.
 * w / b: the nine layers in neo_pix_upload_mlp's order.  tape: neo_pix_mlp_train_tape_floats(NV, P) floats kept between forward and
 * backward.  The backward returns the nine weight / bias gradients (gw / gb ZEROED by the caller; the latent columns of gw[0] stay
 * untouched: their gradient is the texel-space GEMM's), g_pre (R, 128) = dL/dz0 and, when g_x_enc is not null, dL/dx_enc. */
long neo_pix_mlp_train_tape_floats(int NV, long P);
int neo_pix_mlp_train_forward_pre(neo_ctx* ctx, const float* const* w, const float* const* b, const float* x_enc, const float* pre,
                                  const float* cond, int NV, long P, float* tape, float* raw_rgb, float* raw_sigma, int* chain_mode,
                                  void* stream);
int neo_pix_mlp_train_backward_pre(neo_ctx* ctx, const float* const* w, const float* x_enc, const float* cond, int NV, long P,
                                   const float* tape, const float* g_rgb, const float* g_sigma, float* const* gw, float* const* gb,
                                   float* g_x_enc, float* g_pre, int chain_mode, void* stream);
/* Mip-NeRF 360's MLPs under autograd as ONE chain each way (round 6; mipnerf360/model.py:107-176 inside the training step :236-365):
 * rows = R rays x n intervals, x0 (rows, 504) integrated encodings (neo_mip_encode; data, no gradient), d_enc (R, 27) one direction
 * encoding per ray.  width / depth = netwidth / netdepth (256 x 4 proposal, 1024 x 8 NeRF; the layer after index 4 reads [h | x0]),
 * rgb = 0 for the proposal MLPs (disable_rgb: colour columns zero).  w / b in neo_mip_upload_mlp's order.  rgbdens (rows, 4) =
 * [sigmoid(raw) (1 + 2 pad) - pad | softplus(raw_density - 1)], activated as the reference returns them.  tape: caller-owned,
 * neo_mip_mlp_train_tape_floats floats, kept with rgbdens between forward and backward.  Backward: g_rgbdens (rows, 4) = dL/d rgbdens;
 * gw / gb ZEROED by the caller. */
long neo_mip_mlp_train_tape_floats(int width, int depth, int rgb, long R, int n);
int neo_mip_mlp_train_forward(neo_ctx* ctx, int width, int depth, int rgb, const float* const* w, const float* const* b, const float* x0,
                              const float* d_enc, long R, int n, float* tape, float* rgbdens, void* stream);
int neo_mip_mlp_train_backward(neo_ctx* ctx, int width, int depth, int rgb, const float* const* w, const float* x0, const float* d_enc,
                               long R, int n, const float* tape, const float* rgbdens, const float* g_rgbdens, float* const* gw,
                               float* const* gb, void* stream);
/* neo_tp_gather_map / _backward at the PixelNeRF decoder's taps (scene geometry of neo_pix_set_scene). */
int neo_pix_gather_map(neo_ctx* ctx, const float* map, long texels, int C, const float* pts, long P, const float* src_poses, int NV, float focal,
                       float cx, float cy, float* out, void* stream);
int neo_pix_gather_map_backward(neo_ctx* ctx, long texels, int C, const float* pts, long P, const float* src_poses, int NV, float focal, float cx,
                                float cy, const float* g_out, float* g_map, void* stream);

/* Weight (and bias) gradient of a linear layer y = x W^T + b over K rows - what autograd forms for every nn.Linear of the
 * reference's MLPs (torch's addmm backward), here for the texel-space projection of training.project_latent:
 * dW (M, N; row pitch ldw) += dY^T X, db (M) += column sums of dY (db may be NULL).  dY (K, M) row pitch ldy, X (K, N) row pitch
 * ldx, fp32, exact fp32 MFMA; M <= 1024, N <= 4096 (a (texels, 256)^T (texels, 512) product runs at ~110 TFLOP/s). */
int neo_linear_weight_grad(neo_ctx* ctx, int M, int N, long K, const float* dY, long ldy, const float* X, long ldx, float* dW,
                           long ldw, float* db, void* stream);

/* Stand-alone feature lookups of the scene set with neo_tp_set_scene, view-major rows (row = v P + p):
 * world (NV*P,128) = index_grid (encoder_tp_fusion_conv.py:122-209: three planes summed), local (NV*P,512) =
 * get_local_feats / SpatialEncoder.index (neo360/model.py:239-264).  pts (P,3) world points.  local (and, in the backward, g_local
 * together with g_latent) may be NULL: the tri-planes only. */
int neo_tp_gather(neo_ctx* ctx, const float* pts, long P, const float* src_poses, int NV, float focal, float cx,
                  float cy, float* world, float* local, void* stream);
/* Its backward: g_world / g_local scattered (atomic adds) into CHANNELS-LAST gradient maps the caller zeroed:
 * g_plane_* (NV,Hp,Wp,128), g_latent (NV,Hf,Wf,512).  Points carry no gradient. */
int neo_tp_gather_backward(neo_ctx* ctx, const float* pts, long P, const float* src_poses, int NV, float focal,
                           float cx, float cy, const float* g_world, const float* g_local, float* g_plane_xz,
                           float* g_plane_xy, float* g_plane_yz, float* g_latent, void* stream);

/* NeRF_TP.forward in its TRAINING form (neo360/model.py:531-579, out_depth=False): white_bkgd honoured, per level
 * rgb (R,3), fg_weights / bg_weights (R,N), the sample rows fg_tvals / bg_tvals (R,N) the caller derives sdist from
 * (:564-571), bg_acc (R), and optionally the per-sample (rgb, sigma) of both regions (inputs of
 * neo_composite_backward).  seed != 0 = randomized=True: stratified level-0 jitter and uniform level-1 quantiles
 * from neo_rand_uniform streams 0..3; seed == 0 = randomized=False.  Any output pointer may be NULL. */
typedef struct {
    float* rgb; float* fg_weights; float* bg_weights; float* fg_tvals; float* bg_tvals; float* bg_acc;
    float* fg_rgbsigma; float* bg_rgbsigma;
} neo_tp_train_out;
int neo_tp_render_train(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R,
                        int chunk, const float* src_poses, int NV, float focal, float cx, float cy, int n_coarse,
                        int n_fine, int white_bkgd, uint64_t seed, const neo_tp_train_out* level0,
                        const neo_tp_train_out* level1, void* stream);

/* ---- PixelNeRF baseline decoder (models/vanilla_nerf/model_pixel.py) ------------------------ */
/* Upload one NeRFMLP of model_pixel.py:35-94 (slot 0 = coarse_mlp, 1 = fine_mlp).  weights/biases
 * [host arrays of 9 device pointers], order: pts_linears.0..3 (128x575, 128x128 x3), views_linear.0
 * (128x155), views_linear.1 (128x128), bottleneck_layer, density_layer, rgb_layer (3x128).
 * Packs the fragments of both arithmetics (neo_ctx_set_precision): every evaluator of the library, the scene encoder's
 * pillar stage included, has a split-fp16 and an exact-fp32 form. */
int neo_pix_upload_mlp(neo_ctx* ctx, int slot, const float* const* weights,
                       const float* const* biases, void* stream);

/* The image encoder's output the reference recomputes per chunk (model_pixel.py:176-178):
 * latent (NV,512,Hf,Wf) NCHW, re-laid out channels-last into a context-owned buffer. */
int neo_pix_set_scene(neo_ctx* ctx, const float* latent, int NV, int Cl, int Hf, int Wf,
                      float image_w, float image_h, void* stream);

/* enable != 0 (default): the 512-channel latent is pre-projected once per (scene, MLP slot) through the latent columns
 * of pts_linears.0 (model_pixel.py:96-131 is linear in the latent up to the first ReLU) and the evaluator gathers the
 * 128-channel result (512 B per latent texel and slot of context memory); 0: the latent itself is gathered and
 * multiplied per point, the reference's operation order. */
int neo_pix_set_preproject(neo_ctx* ctx, int enable);

/* Per-point outputs at given sample positions (model_pixel.py:198-237): tvals (R,N) along rays_d;
 * out (R,N,4) = (sigmoid rgb, relu sigma).  chunk / src_poses / focal / cx / cy as for neo_pix_render. */
int neo_pix_mlp(neo_ctx* ctx, int slot, const float* rays_o, const float* rays_d,
                const float* viewdirs, const float* tvals, int R, int N, int chunk,
                const float* src_poses, int NV, float focal, float cx, float cy, float* out,
                void* stream);

/* PixelNeRF.forward decoder half (model_pixel.py:180-256), randomized=False, for R rays processed in
 * reference-sized chunks (the view-direction tiling of :219-222 makes results depend on chunk
 * membership).  src_poses [host]: NV*16 floats; focal/cx/cy: source view 0's intrinsics (:203-204;
 * both image axes use +focal).  Outputs per level (any may be NULL): rgb (R,3), acc (R), depth (R). */
int neo_pix_render(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs,
                   int R, int chunk, const float* src_poses, int NV, float focal, float cx,
                   float cy, float near, float far, int n_coarse, int n_fine, int white_bkgd,
                   float* rgb0, float* acc0, float* depth0, float* rgb1, float* acc1,
                   float* depth1, void* stream);

/* PIXELNERF MARCHING FRAME: empty-space skipping and early ray termination for the PixelNeRF baseline decoder.  Given the scene
 * latent, the source cameras and the weights, a PixelNeRF density depends on the position alone, so a grid built once per scene over
 * a caller-given box stays valid for every frame of that scene.  The pieces are those of the VANILLA MARCHING FRAME above (BOX GRID,
 * BOX KEEP RULE, MODE-0 STOP RULE, its BOUND and its samples struct), with two differences: positions lie along rays_d (the keep
 * rule's `dirs` is rays_d), and a sample is SEEN along the direction of the quirk-Q1 ray of the dense launch, ray c0 + ((r - c0) N
 * + j) mod bc of the reference chunk [c0, c0 + bc) of ray r - so a row's value depends on `chunk`, as in neo_pix_render.
 *
 * neo_pix_set_occupancy installs the BOX GRID in a slot of its own (arguments and ordering of neo_vanilla_set_occupancy; bits == NULL
 * removes it).  The grid belongs to the scene latent, the source cameras and the uploaded weights, which the library cannot check.
 * neo_pix_set_march_window: rays per window of neo_pix_render_marching, 1 .. 65536, 0 = the default (16384); results do not depend on it.
 *
 * neo_pix_mlp_compact is neo_pix_mlp on single points whose number lives on the device: rays_o, rays_d, viewdirs (cap,3), t (cap) and
 * out (cap,4) are allocated for `cap` rows, the host's bound, and min(*count_dev, cap) of them are live (count_dev [device]: one int;
 * 0 is a valid launch).  Row k is the point rays_o[k] + t[k] * rays_d[k] seen along viewdirs[k]: the caller has resolved quirk Q1,
 * every row is its own ray (N = 1, one chunk).  Its out row is bitwise what neo_pix_mlp gives the same point and direction, with and
 * without pre-projection and in both arithmetics.  A row at or behind the count is neither read nor written; a workgroup whose first
 * row is at or behind the count leaves before its first barrier.  Checks and src_poses / focal / cx / cy as for neo_pix_mlp.
 *
 * neo_pix_render_marching is neo_pix_render in which a sample is evaluated iff the BOX KEEP RULE of the installed grid keeps it AND it
 * lies in front of its ray's stop.  A sample that is not evaluated has the row (0, 0, 0, 0) and weight exactly 0; an evaluated one
 * goes through the compact launch and is bitwise neo_pix_mlp's at the call's `chunk`.  LEVELS, eps, segment, coarse, use_grid, the
 * BOUND (coarse == 0: a never-stopped ray bitwise equal to the same call at eps == 0, a stopped ray's level-1 rgb within 1.003 trans
 * per channel and its depth within 1.001 far trans), samples0 / samples1 and kept are neo_vanilla_render_marching's.  Without a grid
 * (or use_grid == 0, or every cell set, or a box that holds no sample and clip == 0) at eps == 0 the six outputs are bitwise
 * neo_pix_render's.  coarse != 0 claims no bound.  Results do not depend on the window, the stream, or on whether the frame is one
 * call or the caller's loop over reference chunks.  R == 0 zeroes kept.  No call synchronises the device. */
int neo_pix_set_occupancy(neo_ctx* ctx, const uint32_t* bits, int G, const float* lo, const float* hi, int clip, void* stream);
int neo_pix_set_march_window(neo_ctx* ctx, int rays);
int neo_pix_mlp_compact(neo_ctx* ctx, int slot, const float* rays_o, const float* rays_d, const float* viewdirs, const float* t,
                        int cap, const int* count_dev, const float* src_poses, int NV, float focal, float cx, float cy, float* out,
                        void* stream);
int neo_pix_render_marching(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs, int R, int chunk,
                            const float* src_poses, int NV, float focal, float cx, float cy, float near, float far, int n_coarse,
                            int n_fine, int white_bkgd, float eps, int segment, int coarse, int use_grid, float* rgb0, float* acc0,
                            float* depth0, float* rgb1, float* acc1, float* depth1, const neo_vanilla_march_samples* samples0,
                            const neo_vanilla_march_samples* samples1, long long* kept, void* stream);

/* ---- Mip-NeRF 360 (models/mipnerf360/model.py) -------------------------------- */
/* Upload one MipNeRF360MLP (model.py:30-107).  slot 0..2 = mlps.0, mlps.1 (PropMLP: width 256,
 * depth 4, rgb 0) and mlps.2 (NeRFMLP: width 1024, depth 8, rgb 1) — the shapes the kernels are
 * specialised for.  weights/biases [host arrays of device pointers], order: pts_linear.0..depth-1,
 * density_layer, then (rgb) bottleneck_layer, views_linear.0, rgb_layer.  basis: the module's
 * pos_basis_t buffer, (3,21) row-major. */
int neo_mip_upload_mlp(neo_ctx* ctx, int slot, int width, int depth, int rgb,
                       const float* const* weights, const float* const* biases,
                       const float* basis, void* stream);

/* One proposal-resampling step (model.py:258-310; helper.py:154-243, :337-394), randomized=False:
 * s_prev (R,n_prev+1) / w_prev (R,n_prev) = previous level's normalised distances and weights
 * (level 0: s_prev = [0,1], w_prev = [1]); dilate != 0 applies max_dilate_weights(dilation,
 * domain (0,1), renormalize) and the [1:-1] trims first; logits = anneal*log(w) (-inf on empty
 * intervals).  Outputs sdist (R,n+1) and tdist = 1/(s/far + (1-s)/near) (R,n+1). */
int neo_mip_resample(neo_ctx* ctx, const float* s_prev, const float* w_prev, int R, int n_prev,
                     int dilate, float dilation, float anneal, int n, float near, float far,
                     float* sdist, float* tdist, void* stream);

/* cast_rays (cone, full covariance) + MipNeRF360MLP.forward for the R*n intervals of tdist (R,n+1)
 * (helper.py:278-334, model.py:109-176): out (R,n,4) = (rgb, density); rgb = 0 for a PropMLP. */
int neo_mip_mlp(neo_ctx* ctx, int slot, const float* rays_o, const float* rays_d,
                const float* viewdirs, const float* radii, const float* tdist, int R, int n,
                float* out, void* stream);

/* Schedule of the NeRF MLP (8 x 1024, models/mipnerf360/model.py:30-120) in split-fp16 arithmetic.  mode 1: layer by
 * layer - the encodings of a batch of 16384 intervals are written once as MFMA fragments, the eight trunk layers run as
 * 256 x 256-tile GEMMs whose activations stay in L2 / Infinity Cache between layers (one weight fragment feeds 4 interval
 * tiles), the fused evaluator adds the heads and the colour branch; 160 MB of context memory.  mode 0: the fused
 * evaluator end to end (one weight fragment per 32 intervals).  mode -1 (a fresh context): layer by layer for calls of
 * 8192 intervals or more.  Same arithmetic per product, a different fp32 summation order inside a layer only through
 * the k-step order, which is the same: results agree to the last bits (tests/test_gpu_mip360.py). */
int neo_mip_set_layered(neo_ctx* ctx, int mode);

/* compute_alpha_weights(opaque_background=True) + volumetric_rendering (helper.py:246-274):
 * rgbdens (R,n,4), tdist (R,n+1) -> weights (R,n), rgb (R,3) = sum w c + max(0,1-acc)*bg. */
int neo_mip_composite(neo_ctx* ctx, const float* rgbdens, const float* tdist, const float* rays_d,
                      int R, int n, float bg, float* weights, float* rgb, void* stream);

/* Training-side operators of the Mip-NeRF 360 renderer (mipnerf360/model.py:236-365 under training_step :436-470), for a caller
 * that composes the MLPs from neo_linear_* (training.mip_render_train):
 * neo_mip_resample_u = neo_mip_resample with the caller's quantile table u (n) and, when jitter != NULL, one offset per ray added
 * to it - helper.py:358-365 with single_jitter: u = linspace(0, 1 - u_max, n) + rand(R, 1) * max_jitter.
 * neo_mip_encode: the 504-d integrated positional encoding of the R x n intervals of tdist (R, n + 1) as fp32 rows (R n, 504),
 * reference feature order (helper.py:33-88, 278-334); pos_basis_t (3, 21) device pointer (the MLP's buffer).
 * neo_mip_composite_backward: backward of neo_mip_composite - g_weights (R, n) and g_rgb (R, 3) (either may be NULL) ->
 * g_rgbdens (R, n, 4) = gradients of (rgb, density); sample positions carry no gradient (stop_level_grad). */
int neo_mip_resample_u(neo_ctx* ctx, const float* s_prev, const float* w_prev, int R, int n_prev, int dilate, float dilation,
                       float anneal, int n, const float* u, const float* jitter, float near, float far, float* sdist, float* tdist,
                       void* stream);
int neo_mip_encode(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* radii, const float* tdist,
                   const float* pos_basis_t, int R, int n, float* out, void* stream);
int neo_mip_composite_backward(neo_ctx* ctx, const float* rgbdens, const float* tdist, const float* rays_d, int R, int n, float bg,
                               const float* g_weights, const float* g_rgb, float* g_rgbdens, void* stream);

/* The regularisers of LitMipNeRF360.training_step (mipnerf360/model.py:444-449, :725-741) in linear time per ray.  t (R, N+1) and
 * w (R, N) are the histogram whose loss is taken (the final level's for the interlevel loss), t_env (R, Ne+1) and w_env (R, Ne) a
 * proposal level's; edges do not decrease along a row; 1 <= N, Ne <= 1024.  Inputs and outputs are fp32, every prefix sum,
 * difference and quotient in between is fp64 and each output entry is rounded once; no atomics, results repeat bit for bit.
 *
 * neo_mip_lossfun_outer: helper.py:135-137 (lossfun_outer over inner_outer :116-131 and searchsorted :108-113):
 * loss (R, N) = max(w - w_outer, 0)^2 / (w + eps), w_outer the envelope weight of the proposal bins a fine interval touches,
 * eps = 1.1920929e-07 (helper.py:18).  The reference takes its mean per proposal level (model.py:733). */
int neo_mip_lossfun_outer(neo_ctx* ctx, const float* t, const float* w, const float* t_env, const float* w_env, int R, int N, int Ne,
                          float* loss, void* stream);
/* Backward of neo_mip_lossfun_outer (autograd of helper.py:116-137 with respect to the two weight tensors): upstream g_loss (R, N)
 * -> g_w (R, N), g_w_env (R, Ne); either may be NULL, not both.  The edges carry no gradient (it is zero almost everywhere). */
int neo_mip_lossfun_outer_backward(neo_ctx* ctx, const float* t, const float* w, const float* t_env, const float* w_env,
                                   const float* g_loss, int R, int N, int Ne, float* g_w, float* g_w_env, void* stream);
/* helper.py:141-148 (lossfun_distortion): loss_rays (R) = sum_ij w_i w_j |u_i - u_j| + sum_i w_i^2 (t_{i+1} - t_i) / 3 with u the
 * interval midpoints (the reference takes the mean over rays, model.py:740); grad_w (R, N), or NULL, = d loss_ray / d w.  No
 * gradient with respect to the edges. */
int neo_mip_lossfun_distortion(neo_ctx* ctx, const float* t, const float* w, int R, int N, float* loss_rays, float* grad_w,
                               void* stream);

/* The per-ray extras of an interval histogram - the slot volumetric_rendering leaves open behind `compute_extras`
 * (mipnerf360/helper.py:264-274), built from integrate_weights (:196-203) and sorted_interp (:207-222).  edges (R, n+1) do not
 * decrease along a row, weights (R, n) are non-negative, 1 <= n <= 1024.  near == far == 0: edges are metric distances t already (any
 * histogram); otherwise edges are sdist and t = s_to_t(edges) = 1 / (s / far + (1 - s) / near) (helper.py:168-172) inside the kernel,
 * no (R, n+1) temporary; exactly one of near / far being 0 is an error.  Inputs and outputs are fp32, every prefix sum, difference
 * and quotient in between (s_to_t included) is fp64 and each output entry is rounded once; no atomics, results repeat bit for bit.
 *
 * neo_mip_extras: u (n_u) DEVICE pointer, ascending quantiles in [0, 1], 0 <= n_u <= 8.  Outputs, any of which may be NULL:
 * acc (R) = sum_i w_i;  dist_mean (R) = clip(nan_to_num(sum_i w_i (t_i + t_{i+1}) / 2 / acc, nan=inf), t_0, t_n) - a row without
 * weight returns t_n;  dist_pct (R, n_u) = sorted_interp(u, integrate_weights(w), t) as the reference's two functions compute it:
 * knots [0, min(cumsum(w[:-1]), 1), 1] without renormalisation, the bracket selected by u >= knot, offset =
 * clip(nan_to_num(., 0), 0, 1).  The percentile jumps where u meets a knot at a zero-weight interval. */
int neo_mip_extras(neo_ctx* ctx, const float* edges, const float* weights, int R, int n, float near, float far, const float* u, int n_u,
                   float* acc, float* dist_mean, float* dist_pct /* (R, n_u) */, void* stream);
/* Backward of (acc, dist_mean) with respect to the weights: upstream g_acc (R), g_mean (R), either may be NULL (= zeros) ->
 * g_w (R, n) = g_acc + g_mean ((t_i + t_{i+1}) / 2 - mean) / acc.  On a row with acc == 0 the second term is DEFINED as 0 (autograd
 * of the forward's expression yields NaN there).  Edges and percentiles carry no gradient: the percentile is piecewise linear in w
 * with jumps at zero-weight intervals, and nothing in the reference differentiates it. */
int neo_mip_extras_backward(neo_ctx* ctx, const float* edges, const float* weights, int R, int n, float near, float far,
                            const float* g_acc, const float* g_mean, float* g_w, void* stream);

/* MipNeRF360.forward(batch, train_frac, randomized=False, is_train=False, near, far)
 * (model.py:236-365), 3 levels (n_prop, n_prop, n_nerf samples).  Per level l (any pointer may be
 * NULL): rgb_l (R,3), sdist_l (R,n_l+1), weights_l (R,n_l), rgbdens_l (R,n_l,4) = per-interval
 * (rgb, density). */
typedef struct {
    float* rgb; float* sdist; float* weights; float* rgbdens;
} neo_mip_level_out;
int neo_mip_render(neo_ctx* ctx, const float* rays_o, const float* rays_d, const float* viewdirs,
                   const float* radii, int R, float train_frac, float near, float far, int n_prop,
                   int n_nerf, const neo_mip_level_out* levels /* [3] */, void* stream);

/* ---- profiling aid ---------------------------------------------------------- */
/* Total duration (ms) of the dominant (fused MLP) kernel launches, bracketed with HIP
 * events on the stream they were launched on, since timing was enabled; with the
 * launch count, the points evaluated and their ALGORITHMIC flops (reference
 * formulation, MAC x 2).  Reading synchronises the events. */
int neo_ctx_set_timing(neo_ctx* ctx, int enable);
int neo_ctx_read_timing(neo_ctx* ctx, double* total_ms, int* launches, double* total_points,
                        double* total_flops);
/* The same launches one by one, in launch order: duration (ms), which evaluator ran (kernel_id: 0 unspecified,
 * 1 k_tp_mlp_hp, 2 k_tp_mlp_hpp, 3 k_tp_mlp_h, 4 k_tp_mlp; Mip-NeRF 360: 5 proposal MLP (fused split evaluator), 6 NeRF MLP fused,
 * 7 NeRF MLP layer by layer - one span covers all batches of the call -, 8 exact fp32), points and algorithmic flops of each.  A NeO-360 frame is four
 * launches (inside / outside the sphere x coarse / fine) and, in pre-projection mode 3, two different kernels: the bench's
 * roofline object prices each kernel with ITS launches.  The two compact background launches of neo_tp_render_culled and the two
 * compact launches of neo_tp_render_objects (and the 2 K of neo_tp_render_instances) record points = flops = 0: how many rows they evaluated is known on the device only.  Arrays may be NULL; *count = launches recorded (may exceed capacity). */
int neo_ctx_read_spans(neo_ctx* ctx, int capacity, double* ms, int* kernel_id, double* points, double* flops, int* count);

#ifdef __cplusplus
}
#endif
#endif /* NEO360_HIP_H */
