"""Empty-space skipping and early ray termination for the vanilla renderer (include/neo360_hip.h: VANILLA MARCHING FRAME).

`MarchingNeRF` is `models.NeRF` - same constructor, `state_dict` keys and `forward` - with an occupancy grid over a caller-given
box and `render_marching`, the frame in which a sample is evaluated iff the grid keeps it AND it lies in front of the ray's stop.
The stage functions expose the rules the frame is made of, on caller rows:

    occupancy_keep_box          the BOX KEEP RULE (neo_vanilla_occupancy_keep)
    occupancy_from_sigma_box    a lattice of densities -> a grid, no unit-sphere clip (neo_occupancy_from_sigma_box)
    termination_stops_vanilla   the MODE-0 STOP RULE (neo_vanilla_termination_stops)
    eval_points                 the compact evaluator launch: single points under a device count (neo_vanilla_mlp_compact)
    render_marching_rays        the frame helper

and, for training through the grid (VANILLA MARCHING TRAINING: `MarchingNeRF.render_train_marching`, `init_occupancy`,
`update_occupancy`):

    train_rows                  the compact row builder: keep mask, device count, indices, encodings (neo_vanilla_train_rows)
    nerf_mlp_rows               `training.nerf_mlp` on K rows with a cond row each, under autograd
    scatter_activate            activations + scatter into the composite's rows, under autograd (neo_vanilla_train_scatter)
    occupancy_probes            one jittered probe point per cell (neo_vanilla_grid_probes)

`MarchingPixelNeRF` is `models.PixelNeRF` with the same grid and frame (PIXELNERF MARCHING FRAME): positions lie along rays_d, a
sample is seen along the direction the reference's chunk tiling gives it, and `eval_points_pix` is its compact evaluator launch
(neo_pix_mlp_compact).  The first three rules above are reused as they are (`occupancy_keep_box` with dirs = rays_d).

Every caller tensor goes through `context.dense` / `context.owned_output`; a bad shape, dtype, G, box, eps or segment raises
ValueError before any device access.
"""
import ctypes
import math

import torch

from . import _lib, models, ops
from .context import dense, f32, get_context, owned_output, ptr, ptr_table, ray_rows


def _check_box(box, who):
    """box = (lo, hi), three finite numbers each with lo < hi on every axis -> two tuples of floats.  Touches no device."""
    try:
        lo, hi = box
        lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    except (TypeError, ValueError):
        raise ValueError("%s: box must be (lo, hi) with three numbers each, got %r" % (who, box)) from None
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("%s: box must be (lo, hi) with three numbers each, got %r" % (who, box))
    for a in range(3):
        if not (math.isfinite(lo[a]) and math.isfinite(hi[a]) and lo[a] < hi[a]):
            raise ValueError("%s: box needs finite lo < hi on every axis, got %r" % (who, box))
    return tuple(lo), tuple(hi)


def _c3(v):
    return (ctypes.c_float * 3)(*v)


def _rows(rays_o, dirs, t, who):
    """rays_o (B,3) defines B and the device, dirs (B,3), t (B,N) with N >= 1: as the library reads them."""
    rays_o = dense(rays_o, "rays_o", (None, 3))
    B = rays_o.shape[0]
    dirs = dense(dirs, "dirs", (B, 3), device=rays_o.device)
    t = dense(t, "t", (B, None), device=rays_o.device)
    if t.shape[1] < 1:
        raise ValueError("%s: at least one sample per ray" % who)
    return rays_o, dirs, t


@torch.no_grad()
def occupancy_keep_box(occ, box, rays_o, dirs, t, clip=False, ctx=None):
    """The BOX KEEP RULE of `MarchingNeRF.render_marching` on caller rows (neo_vanilla_occupancy_keep): occ bool (G,G,G) on any
    device over the box (lo, hi), or None for "no grid"; rays_o, dirs (B,3) and t (B,N) on the GPU.  Sample j of ray b, at
    x = rays_o[b] + t[b, j] * dirs[b] in fp32, is kept iff a coordinate of x is not finite, or occ is None, or x lies outside the box
    and clip is false, or x lies inside and its cell - per axis floor((x - lo) * (G / (hi - lo))), the scale formed once in fp32 -
    is set.  Returns (B,N) bool."""
    G = 0
    lo = hi = (0.0, 0.0, 0.0)
    if occ is not None:
        G = ops._check_occupancy(occ, "occupancy_keep_box")
        lo, hi = _check_box(box, "occupancy_keep_box")
    rays_o, dirs, t = _rows(rays_o, dirs, t, "occupancy_keep_box")
    B, N = t.shape
    ctx = ops._ctx(t, ctx)
    bits = ops.pack_occupancy(occ.to(t.device)) if occ is not None else None
    keep = torch.empty(B, N, dtype=torch.bool, device=t.device)
    _lib.check(ctx.lib.neo_vanilla_occupancy_keep(ctx.handle, ptr(bits), G, _c3(lo), _c3(hi), int(bool(clip)), ptr(rays_o), ptr(dirs),
                                                  ptr(t), B, N, keep.data_ptr(), ctx.stream()))
    return keep


def occupancy_lattice_box(box, resolution, probes, device="cpu"):
    """The probe positions of `MarchingNeRF.build_occupancy`: per axis the M = resolution * probes sub-centres
    lo + (l + 1/2) (hi - lo) / M (fp64, rounded to fp32), and the lattice as rays - column (lx, ly) is the ray
    o = (cx[lx], cy[ly], 0), d = (0, 0, 1) sampled at t = cz, so that o + t d is the lattice point exactly.
    Returns (cz (M,), rays_o (M^2,3), rays_d (M^2,3))."""
    lo, hi = _check_box(box, "occupancy_lattice_box")
    M = int(resolution) * int(probes)
    c = [(lo[a] + (torch.arange(M, dtype=torch.float64) + 0.5) * ((hi[a] - lo[a]) / M)).float().to(device) for a in range(3)]
    rays_o = torch.stack([c[0][:, None].expand(M, M), c[1][None, :].expand(M, M), torch.zeros(M, M, device=device)], dim=-1)
    rays_d = torch.tensor([0.0, 0.0, 1.0], device=device).expand(M * M, 3).contiguous()
    return c[2], rays_o.reshape(M * M, 3).contiguous(), rays_d


@torch.no_grad()
def occupancy_from_sigma_box(sigma, resolution, sigma_threshold, probes=2, dilate=1, ctx=None):
    """A lattice of activated densities over a box -> a bool (G,G,G) grid (neo_occupancy_from_sigma_box): `ops.occupancy_from_sigma`
    without its unit-sphere clip.  sigma: (M,M,M) on the GPU, M = resolution * probes, entry (lx, ly, lz) a probe of cell
    (lx // probes, ly // probes, lz // probes).  A cell is occupied iff a probe of a cell within `dilate` cells of it in every axis
    is not <= sigma_threshold (a NaN density is occupied)."""
    G, probes, dilate = ops._check_build(resolution, sigma_threshold, probes, dilate, "occupancy_from_sigma_box")
    M = G * probes
    sigma = dense(sigma, "sigma", (M, M, M))
    ctx = ops._ctx(sigma, ctx)
    bits = torch.empty(G ** 3 // 32, dtype=torch.int32, device=sigma.device)
    _lib.check(ctx.lib.neo_occupancy_from_sigma_box(ctx.handle, ptr(sigma), G, probes, float(sigma_threshold), dilate, ptr(bits),
                                                    ctx.stream()))
    return ops.unpack_occupancy(bits, G)


@torch.no_grad()
def termination_stops_vanilla(rgbsigma, t, rays_d, eps, segment=64, ctx=None):
    """The MODE-0 STOP RULE of `MarchingNeRF.render_marching` on caller rows (neo_vanilla_termination_stops): rgbsigma (B,N,4),
    t (B,N), rays_d (B,3) on the GPU - what `eval_mlp` returns and what `ops.composite(0, ...)` reads.  The N samples are cut into
    segments of `segment` (a positive multiple of 64); a march evaluates segment 0, and segment k >= 1 iff at every earlier boundary
    b the transmittance in front of sample b - the composite's own (float)carry, formed with its expressions: the last interval is
    1e10 and every interval is scaled by |rays_d| - was not below eps (a NaN keeps marching).  Returns (stop (B,) int32, the leading
    samples such a march evaluates, and trans (B,) float32, the transmittance at the stop)."""
    eps, segment = ops._check_termination(eps, segment, "termination_stops_vanilla")
    t = dense(t, "t", (None, None))
    B, N = t.shape
    if N < 1:
        raise ValueError("termination_stops_vanilla: at least one sample per ray")
    rgbsigma = dense(rgbsigma, "rgbsigma", (B, N, 4), device=t.device)
    rays_d = dense(rays_d, "rays_d", (B, 3), device=t.device)
    ctx = ops._ctx(t, ctx)
    stop = torch.empty(B, dtype=torch.int32, device=t.device)
    trans = torch.empty(B, device=t.device)
    _lib.check(ctx.lib.neo_vanilla_termination_stops(ctx.handle, ptr(rgbsigma), ptr(t), ptr(rays_d), B, N, eps, segment,
                                                     stop.data_ptr(), trans.data_ptr(), ctx.stream()))
    return stop, trans


@torch.no_grad()
def eval_points(model, level, rays_o, dirs, t, count, out=None):
    """The compact evaluator launch (neo_vanilla_mlp_compact): `model.eval_mlp(level, ...)` on single points whose number lives on
    the device.  rays_o, dirs (cap,3) and t (cap,) on the GPU are allocated for `cap` rows, of which min(count, cap) are live;
    count is an int32 device tensor of one element and is not read by the host.  Row k is the point rays_o[k] + t[k] * dirs[k] seen
    along dirs[k]; its (rgb, sigma) row is bitwise `eval_mlp`'s for that point.  out: a caller-owned (cap,4) float32 tensor, written
    in place - rows at or behind the count stay as they are - or None for a fresh one (whose rows behind the count are undefined).
    Returns out."""
    if not isinstance(model, models.NeRF):
        raise TypeError("eval_points evaluates NeRF modules, got %r" % type(model))
    if level not in (0, 1):
        raise ValueError("eval_points: level must be 0 or 1, got %r" % (level,))
    rays_o = dense(rays_o, "rays_o", (None, 3))
    cap, dev = rays_o.shape[0], rays_o.device
    dirs = dense(dirs, "dirs", (cap, 3), device=dev)
    t = dense(t, "t", [(cap,), (cap, 1)], device=dev)
    count = dense(count, "count", [(), (1,)], dtypes=(torch.int32,), to=torch.int32, device=dev)
    if out is None:
        out = torch.empty(cap, 4, device=dev)
    else:
        out = owned_output(out, "out", (cap, 4), device=dev)
        _lib.note_external_write()
    ctx = model._context(dev)
    model._sync_weights(ctx)
    _lib.check(ctx.lib.neo_vanilla_mlp_compact(ctx.handle, int(level), ptr(rays_o), ptr(dirs), ptr(t), cap, ptr(count), ptr(out),
                                               ctx.stream()))
    model._raise_flags(ctx.poll_flags())     # stage-level access: always immediate
    return out


@torch.no_grad()
def eval_points_pix(model, slot, rays, t, count, out=None):
    """The compact launch of the PixelNeRF evaluators (neo_pix_mlp_compact): `model.eval_mlp(slot, ...)` on single points whose
    number lives on the device.  rays["rays_o" | "rays_d" | "viewdirs"] (cap,3) and t (cap,) or (cap,1) on the GPU are allocated for
    `cap` rows, of which min(count, cap) are live; rays also carries the source cameras (`src_poses`, `src_focal`, `src_c`; `src_imgs`
    for an attached encoder).  count is an int32 device tensor of one element and is not read by the host.  Row k is the point
    rays_o[k] + t[k] * rays_d[k] seen along viewdirs[k] - the caller has resolved the reference's direction tiling, every row is
    its own ray; its (rgb, sigma) row is bitwise `eval_mlp`'s for that point and direction, with and without `preproject` and in
    both arithmetics.  out: a caller-owned (cap,4) float32 tensor, written in place - rows at or behind the count stay as they
    are - or None for a fresh one (whose rows behind the count are undefined).  Returns out."""
    if not isinstance(model, models.PixelNeRF):
        raise TypeError("eval_points_pix evaluates PixelNeRF modules, got %r" % type(model))
    if slot not in (0, 1):
        raise ValueError("eval_points_pix: slot must be 0 or 1, got %r" % (slot,))
    rays_o, rays_d, viewdirs = ray_rows(rays)
    cap, dev = rays_o.shape[0], rays_o.device
    t = dense(t, "t", [(cap,), (cap, 1)], device=dev)
    count = dense(count, "count", [(), (1,)], dtypes=(torch.int32,), to=torch.int32, device=dev)
    if out is None:
        out = torch.empty(cap, 4, device=dev)
    else:
        out = owned_output(out, "out", (cap, 4), device=dev)
        _lib.note_external_write()
    ctx = model._context(dev)
    model._ensure_scene(rays)
    model._sync_weights(ctx)
    host_poses, NV, focal, cx, cy = model._camera_args(rays)
    _lib.check(ctx.lib.neo_pix_mlp_compact(ctx.handle, int(slot), ptr(rays_o), ptr(rays_d), ptr(viewdirs), ptr(t), cap, ptr(count),
                                           host_poses, NV, focal, cx, cy, ptr(out), ctx.stream()))
    model._raise_flags(ctx.poll_flags())     # stage-level access: always immediate
    return out


# ---- training through the grid (include/neo360_hip.h: VANILLA MARCHING TRAINING) ----------------------------------------------

def _train_rows(ctx, bits, G, lo, hi, clip, rays_o, dirs, t, dir_enc, out=None):
    """neo_vanilla_train_rows on converted tensors and packed bits (None: no grid)."""
    B, N = t.shape
    dev = t.device
    cap = B * N
    keep = torch.empty(B, N, dtype=torch.bool, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    if out is None:
        index = torch.empty(cap, dtype=torch.int32, device=dev)
        x_enc, cond = torch.empty(cap, 63, device=dev), torch.empty(cap, 27, device=dev)
    else:
        index, x_enc, cond = out
    _lib.check(ctx.lib.neo_vanilla_train_rows(ctx.handle, ptr(bits), G, _c3(lo), _c3(hi), int(bool(clip)), ptr(rays_o), ptr(dirs), ptr(t),
                                              ptr(dir_enc), B, N, cap, keep.data_ptr(), count.data_ptr(), index.data_ptr(),
                                              x_enc.data_ptr(), cond.data_ptr(), ctx.stream()))
    return keep, count, index, x_enc, cond


@torch.no_grad()
def train_rows(occ, box, rays_o, dirs, t, dir_enc, clip=False, ctx=None, out=None):
    """The compact row builder of `MarchingNeRF.render_train_marching` on caller rows (neo_vanilla_train_rows): occ / box / clip as
    `occupancy_keep_box` takes them (occ None: no grid), rays_o, dirs (B,3), t (B,N) and dir_enc (B,27) on the GPU.  Returns
    (keep bool (B,N) - the BOX KEEP RULE -, count int32[1] ON THE DEVICE - the kept samples, not read here -, index int32 (B N,),
    x_enc (B N, 63), cond (B N, 27)): for k < count, in ascending flat order, index[k] = b N + j of the k-th kept sample, x_enc[k]
    bitwise `ops.pos_enc(rays_o[b] + t[b, j] * dirs[b], 0, 10)` and cond[k] = dir_enc[b].  The last three are allocated for B N rows;
    rows at or behind the count are neither read nor written (out = (index, x_enc, cond): caller-owned tensors of those shapes,
    written in place, so that a caller can see it).  No atomics, nothing synchronises."""
    G = 0
    lo = hi = (0.0, 0.0, 0.0)
    if occ is not None:
        G = ops._check_occupancy(occ, "train_rows")
        lo, hi = _check_box(box, "train_rows")
    rays_o, dirs, t = _rows(rays_o, dirs, t, "train_rows")
    B, N = t.shape
    dir_enc = dense(dir_enc, "dir_enc", (B, 27), device=t.device)
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 3:
            raise ValueError("train_rows: out must be the three tensors (index, x_enc, cond)")
        out = (owned_output(out[0], "out[0] (index)", (B * N,), dtype=torch.int32, device=t.device),
               owned_output(out[1], "out[1] (x_enc)", (B * N, 63), device=t.device),
               owned_output(out[2], "out[2] (cond)", (B * N, 27), device=t.device))
        _lib.note_external_write()
    ctx = ops._ctx(t, ctx)
    bits = ops.pack_occupancy(occ.to(t.device)) if occ is not None else None
    return _train_rows(ctx, bits, G, lo, hi, clip, rays_o, dirs, t, dir_enc, out)


_NERF_LAYER_SHAPES = [(256, 63)] + [(256, 256)] * 4 + [(256, 319)] + [(256, 256)] * 2 + [(128, 283), (256, 256), (1, 256), (3, 128)]


class _TrainVanillaRows(torch.autograd.Function):
    """Vanilla NeRFMLP on K caller rows, each with its own cond (neo_vanilla_mlp_train_forward / _backward with R = K)."""

    @staticmethod
    def forward(ctx_, lib_ctx, x_enc, cond, *params):
        from . import training as T
        ws, bs = params[:12], params[12:]
        x0 = dense(x_enc, "x_enc", (None, 63))      # x_enc defines K and the device
        K, dev = x0.shape[0], x0.device
        cd = dense(cond, "cond", (K, 27), device=dev)
        T._check_layers("NeRFMLP layer", ws, bs, _NERF_LAYER_SHAPES)
        raw_rgb, raw_sigma = torch.empty(K, 3, device=dev), torch.empty(K, 1, device=dev)
        ctx_.meta = (None, K)
        if K == 0:      # nothing to evaluate: the library is not called, and the backward returns exact zeros
            ctx_.save_for_backward(*[w.detach() for w in ws])
            return raw_rgb, raw_sigma
        c = ops._ctx(x0, lib_ctx)
        wd, bd = T._detached(ws, bs)
        tape = torch.empty(c.lib.neo_vanilla_mlp_train_tape_floats(K), device=dev)
        _lib.check(c.lib.neo_vanilla_mlp_train_forward(c.handle, ptr_table(wd), ptr_table(bd), ptr(x0), ptr(cd), K, ptr(tape),
                                                       ptr(raw_rgb), ptr(raw_sigma), c.stream()))
        ctx_.save_for_backward(x0, cd, tape, *wd)
        ctx_.meta = (c, K)
        return raw_rgb, raw_sigma

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx_, g_rgb, g_sigma):
        from . import training as T
        c, K = ctx_.meta
        if K == 0:
            wd = ctx_.saved_tensors
            gw, gb = T._zero_param_grads(wd)
            return (None, torch.zeros(0, 63, device=wd[0].device) if ctx_.needs_input_grad[1] else None, None, *gw, *gb)
        x0, cd, tape, *wd = ctx_.saved_tensors
        if ctx_.needs_input_grad[2]:
            raise NotImplementedError("nerf_mlp_rows: no gradient for cond (the view-direction encodings are data)")
        g_rgb = T._grad_or_zeros(g_rgb, "g_rgb", K, 3, x0.device)
        g_sigma = T._grad_or_zeros(g_sigma, "g_sigma", K, 1, x0.device)
        gw, gb = T._zero_param_grads(wd)
        g_x0 = torch.empty_like(x0) if ctx_.needs_input_grad[1] else None
        _lib.check(c.lib.neo_vanilla_mlp_train_backward(c.handle, ptr_table(wd), ptr(x0), ptr(cd), K, ptr(tape), ptr(g_rgb),
                                                        ptr(g_sigma), ptr_table(gw), ptr_table(gb), ptr(g_x0), None, c.stream()))
        return (None, g_x0, None, *gw, *gb)


def nerf_mlp_rows(mlp, x_enc, cond, ctx=None):
    """The row form of `training.nerf_mlp`: x_enc (K,63) encoded points and cond (K,27), each row's own view-direction encoding
    (what `train_rows` emits) -> raw_rgb (K,3), raw_sigma (K,1).  Gradients flow to the 24 parameter tensors of `mlp`
    (a models.NeRFMLP) and to x_enc.  K == 0 returns empty outputs and, in the backward, exact-zero parameter gradients, without
    calling the library.  Exact fp32 matrix arithmetic."""
    from . import training as T
    if not isinstance(mlp, models.NeRFMLP):
        raise TypeError("nerf_mlp_rows evaluates NeRFMLP containers, got %r" % type(mlp))
    return _TrainVanillaRows.apply(ctx, x_enc, cond, *T._mlp_params(mlp))


class _ScatterActivate(torch.autograd.Function):
    @staticmethod
    def forward(ctx_, raw_rgb, raw_sigma, index, total, noise, noise_scale, lib_ctx):
        if isinstance(total, bool) or not isinstance(total, int) or total < 0:
            raise ValueError("scatter_activate: total must be a non-negative integer, got %r" % (total,))
        index = dense(index, "index", (None,), dtypes=(torch.int32,), to=torch.int32)      # index defines K and the device
        K, dev = index.shape[0], index.device
        if K > total:
            raise ValueError("scatter_activate: %d rows cannot be scattered into %d" % (K, total))
        raw_rgb = dense(raw_rgb, "raw_rgb", (K, 3), device=dev)
        raw_sigma = dense(raw_sigma, "raw_sigma", [(K,), (K, 1)], device=dev)
        noise = dense(noise, "noise", device=dev) if noise is not None else None
        if noise is not None and noise.numel() != total:
            raise ValueError("noise must hold one value per point (%d), got %s" % (total, tuple(noise.shape)))
        c = ops._ctx(index, lib_ctx)
        packed = torch.empty(total, 4, device=dev)
        _lib.check(c.lib.neo_vanilla_train_scatter(c.handle, ptr(raw_rgb), ptr(raw_sigma), ptr(index), K, ptr(noise), float(noise_scale),
                                                   total, ptr(packed), c.stream()))
        ctx_.save_for_backward(raw_rgb, raw_sigma, index, noise if noise is not None else torch.empty(0, device=dev))
        ctx_.meta = (c, float(noise_scale), noise is not None, total, tuple(raw_sigma.shape))
        return packed

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx_, g):
        raw_rgb, raw_sigma, index, noise = ctx_.saved_tensors
        c, scale, has_noise, total, shape_sigma = ctx_.meta
        K = index.shape[0]
        g_rgb, g_sigma = torch.empty(K, 3, device=index.device), torch.empty(K, device=index.device)
        if K:
            g = f32(g.reshape(total, 4).contiguous(), "grad")
            _lib.check(c.lib.neo_vanilla_train_scatter_backward(c.handle, ptr(raw_rgb), ptr(raw_sigma), ptr(index), K,
                                                                ptr(noise) if has_noise else None, scale, total, ptr(g), ptr(g_rgb),
                                                                ptr(g_sigma), c.stream()))
        return g_rgb, g_sigma.reshape(shape_sigma), None, None, None, None, None


def scatter_activate(raw_rgb, raw_sigma, index, total, noise=None, noise_scale=0.0, ctx=None):
    """`training.activate` fused with the scatter into the composite's rows (neo_vanilla_train_scatter / _backward): raw_rgb (K,3),
    raw_sigma (K,) or (K,1), index int32 (K,) - distinct flat positions in [0, total) - and optionally noise, `total` uniforms
    indexed by POSITION -> packed (total, 4): row index[k] is bitwise `training.activate`'s row of (raw_rgb[k], raw_sigma[k],
    noise[index[k]]), every other row is zero (composite mode 0 gives such a sample weight exactly 0).  The backward gathers the
    gradient rows at index and is bitwise `training.activate`'s on them.  K == 0: all zeros, empty gradients."""
    return _ScatterActivate.apply(raw_rgb, raw_sigma, index, total, noise, noise_scale, ctx)


def _check_counter(v, name, who, bits):
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** bits:
        raise ValueError("%s: %s must be an integer in [0, 2^%d), got %r" % (who, name, bits, v))
    return v


@torch.no_grad()
def occupancy_probes(box, resolution, seed, step, device="cuda", ctx=None):
    """The probe points of `MarchingNeRF.update_occupancy` (neo_vanilla_grid_probes): (G^3, 3), G = resolution, in the grid's
    [ix][iy][iz] order - one point per cell of the grid over box = (lo, hi), at lo + (c + u) (hi - lo) / G per axis, u in [0, 1) from
    the library's counter-based generator (key `seed`, counter (cell, step, 8 + axis, 0)).  Every point lies in its own cell under
    the grid's fp32 cell expression (`occupancy_keep_box`); a candidate that rounding pushed over a face is replaced by the cell's
    centre on that axis.  The same (seed, step) gives the same bits."""
    if not ops.occupancy_resolution_ok(resolution):
        raise ValueError("occupancy_probes: resolution must be 8, 16 or a multiple of 32 in [32, 256], got %r" % (resolution,))
    lo, hi = _check_box(box, "occupancy_probes")
    seed = _check_counter(seed, "seed", "occupancy_probes", 64)
    step = _check_counter(step, "step", "occupancy_probes", 32)
    G = int(resolution)
    for a in range(3):      # the library's own refusal, before any device access
        lo32, hi32 = (torch.tensor(v, dtype=torch.float32) for v in (lo[a], hi[a]))
        if not float((hi32 - lo32) / G) * 131072.0 >= max(abs(float(lo32)), abs(float(hi32))):
            raise ValueError("occupancy_probes: the box's cells are too thin for fp32 probe points, got %r" % (box,))
    if ctx is None:
        ctx = get_context(device)
    pts = torch.empty(G ** 3, 3, device=ctx.device)
    _lib.check(ctx.lib.neo_vanilla_grid_probes(ctx.handle, G, _c3(lo), _c3(hi), seed, step, ptr(pts), ctx.stream()))
    return pts


class _BoxOccupancy:
    """The installed box grid of a marching module: the module's copy, its box and clip, and the library context that holds the
    bits (`_occ_entry`: that renderer's set_occupancy entry point)."""

    _occ_entry = None

    def _init_box_occupancy(self):
        self._occupancy = self._occ_box = self._occ_ctx = None
        self._occ_clip = False
        self._occ_bits = None
        self.last_march_kept = None

    @property
    def occupancy(self):
        """The installed occupancy grid as a bool (G,G,G) device tensor (a copy), or None."""
        return None if self._occupancy is None else self._occupancy.clone()

    @property
    def occupancy_box(self):
        """(lo, hi) of the installed grid, two tuples of three floats, or None."""
        return self._occ_box

    @torch.no_grad()
    def set_occupancy(self, grid, box=None, clip=False):
        """Installs (or, with grid None, removes) the grid `render_marching` reads: a bool (G,G,G) tensor on any device, indexed
        [ix, iy, iz], over box = (lo, hi) - three finite numbers each, lo < hi; G is 8, 16 or a multiple of 32 in [32, 256].
        clip=False keeps a sample outside the box, clip=True skips it.  ValueError - before any device access - for another shape,
        dtype, G or box.  The grid is copied to the module's device and, as bits, into the library context.  It belongs to the
        weights of both MLPs, which the module cannot check: install a new grid (`build_occupancy`) whenever they change."""
        if grid is None:
            if self._occ_ctx is not None and self._occ_ctx.handle:
                c = self._occ_ctx
                _lib.check(getattr(c.lib, self._occ_entry)(c.handle, None, 0, None, None, 0, c.stream()))
            self._occupancy = self._occ_box = self._occ_ctx = self._occ_bits = None
            self._occ_clip = False
            return
        G = ops._check_occupancy(grid, "set_occupancy")
        lo, hi = _check_box(box, "set_occupancy")
        dev = next(self.parameters()).device
        ctx = self._context(dev)
        occ = grid.detach().to(dev).contiguous().clone()
        bits = ops.pack_occupancy(occ)
        _lib.check(getattr(ctx.lib, self._occ_entry)(ctx.handle, ptr(bits), G, _c3(lo), _c3(hi), int(bool(clip)), ctx.stream()))
        self._occupancy, self._occ_box, self._occ_clip, self._occ_ctx = occ, (lo, hi), bool(clip), ctx
        self._occ_bits = bits       # the training row builder reads the caller-side bits (render_train_marching)


class MarchingNeRF(_BoxOccupancy, models.NeRF):
    """`models.NeRF` with an occupancy grid over a box, the marching frame, and training through the grid
    (`render_train_marching`, `init_occupancy`, `update_occupancy`).  `forward`, `eval_mlp` and the parent's training path read none
    of this."""

    # rays per window of render_marching (None: the library's default, 8192): a window bounds the extra workspace at 68 bytes per
    # (ray, sample) of one window and segment; results do not depend on it
    march_window = None
    _occ_entry = "neo_vanilla_set_occupancy"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._init_box_occupancy()
        self.last_train_kept = None
        self._run = None            # init_occupancy: dict(box, G, clip, density, updates)

    @property
    def occupancy_density(self):
        """The running density of `update_occupancy` as a float (G,G,G) device tensor (a copy), or None before `init_occupancy`."""
        return None if self._run is None else self._run["density"].clone()

    @torch.no_grad()
    def init_occupancy(self, box, resolution, clip=False):
        """Starts a running grid over box = (lo, hi): installs an all-ones grid of `resolution` cells per axis (`set_occupancy`: every
        sample inside the box is kept until the first update) and creates the zero running density (G,G,G) that
        `update_occupancy` maintains (`occupancy_density`).  ValueError, before any device access, for a bad box or resolution."""
        if not ops.occupancy_resolution_ok(resolution):
            raise ValueError("init_occupancy: resolution must be 8, 16 or a multiple of 32 in [32, 256], got %r" % (resolution,))
        G = int(resolution)
        box = _check_box(box, "init_occupancy")
        dev = next(self.parameters()).device
        self.set_occupancy(torch.ones(G, G, G, dtype=torch.bool, device=dev), box, clip)
        self._run = dict(box=box, G=G, clip=bool(clip), density=torch.zeros(G, G, G, device=dev), updates=0)

    @torch.no_grad()
    def update_occupancy(self, sigma_threshold, decay=0.95, dilate=1, seed=1):
        """One update of the running grid of `init_occupancy`, from the module's CURRENT parameters: one jittered probe point per
        cell (`occupancy_probes` with step = the number of updates so far), both MLPs evaluated there through the compact evaluator
        (`eval_points`; a vanilla density depends on the position alone), density = max(decay * density, max(sigma_0, sigma_1))
        per cell (neo_vanilla_density_update; a NaN stays), and the grid = `occupancy_from_sigma_box(density, G, sigma_threshold,
        probes=1, dilate)`, installed with `set_occupancy` and returned.  EVERY cell is probed at every update, whatever the current
        grid says: a cleared cell comes back as soon as its density does, and an emptied one clears once decay^n has taken its
        remembered density to the threshold.  sigma_threshold has no default: nobody has measured one on trained weights.
        ValueError, before any device access, for a bad threshold, decay (outside [0, 1]), dilate or seed; NeoError before
        `init_occupancy`."""
        if self._run is None:
            raise _lib.NeoError("update_occupancy: no running grid - call init_occupancy(box, resolution) first")
        run = self._run
        G, _, dilate = ops._check_build(run["G"], sigma_threshold, 1, dilate, "update_occupancy")
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) <= 1.0:
            raise ValueError("update_occupancy: decay must be a number in [0, 1], got %r" % (decay,))
        seed = _check_counter(seed, "seed", "update_occupancy", 64)
        dev = next(self.parameters()).device
        if run["density"].device != dev:
            raise _lib.NeoError("the running density lives on %s, the module on %s: call init_occupancy again" % (run["density"].device, dev))
        ctx = self._context(dev)
        cells = G ** 3
        pts = occupancy_probes(run["box"], G, seed, run["updates"] & 0xFFFFFFFF, ctx=ctx)
        dirs = torch.zeros(cells, 3, device=dev)
        dirs[:, 2] = 1.0
        t = torch.zeros(cells, device=dev)
        count = torch.full((1,), cells, dtype=torch.int32, device=dev)
        sigma = [eval_points(self, lv, pts, dirs, t, count)[:, 3].contiguous() for lv in range(2)]
        _lib.check(ctx.lib.neo_vanilla_density_update(ctx.handle, ptr(run["density"]), ptr(sigma[0]), ptr(sigma[1]), G, float(decay),
                                                      ctx.stream()))
        grid = occupancy_from_sigma_box(run["density"], G, sigma_threshold, probes=1, dilate=dilate, ctx=ctx)
        self.set_occupancy(grid, run["box"], run["clip"])
        run["updates"] += 1
        return grid

    def render_train_marching(self, rays, randomized, white_bkgd, near, far, seed=None, grid=True, return_samples=False):
        """`training.nerf_render_train(self, rays, randomized, white_bkgd, near, far, seed)` - the same sample positions, random
        streams, noise tables, composite and resampling - in which only the samples the installed grid keeps (`occupancy_keep_box`;
        grid=False or no grid: every sample) go through the MLP, forward and backward.  Per level, between the positions and the
        composite: `train_rows` (keep mask, count, flat indices, encodings and direction rows of the kept samples), ONE 4-byte read
        of the count, `nerf_mlp_rows` on exactly that many rows, `scatter_activate` into the level's zero rows.  A sample that is
        not kept has the row (0, 0, 0, 0): weight exactly 0, no gradient.  There is no stop rule here: a training ray must see its
        whole interval.  Without a grid (or with every cell set, or a box that holds no sample and clip=False) the six outputs
        are bitwise `nerf_render_train`'s for the same seed.

        The count read BLOCKS, once per level - the training GEMMs take their row count from the host - on top of the flag read at
        the end of the call, which blocks as in `nerf_render_train`.  `self.last_train_kept` = (kept at level 0, kept at level 1)
        as Python ints.  NeoError when grid=True and the installed grid belongs to another context.

        Returns [(rgb (B,3), acc (B,), depth (B,))] * 2; with return_samples (that, [(t (B,N), keep (B,N) bool)] * 2)."""
        from . import training as T
        rays_o, rays_d, viewdirs = ray_rows(rays)        # rays_o defines B
        B, dev = rays_o.shape[0], rays_o.device
        c = self._context(dev)
        use = bool(grid) and self._occupancy is not None
        if use and self._occ_ctx is not c:
            raise _lib.NeoError("the occupancy grid does not belong to this module's context on %s: install it again" % dev)
        bits, G, clip = (self._occ_bits, self._occupancy.shape[0], self._occ_clip) if use else (None, 0, False)
        lo, hi = self._occ_box if use else ((0.0,) * 3, (0.0,) * 3)
        n0, n1 = self.num_coarse_samples, self.num_fine_samples
        noise = float(self.noise_std) if randomized else 0.0
        with torch.no_grad():       # positions and direction encodings: nerf_render_train's own lines
            if randomized:
                seed = int(seed) if seed is not None else int(torch.randint(1, 2 ** 62, (1,)).item())
                seed = seed or 1
            lin = torch.linspace(0.0, 1.0, n0 + 1).to(dev)
            edges = float(near) * (1.0 - lin) + float(far) * lin
            if randomized:
                mids = 0.5 * (edges[1:] + edges[:-1])
                upper, lower = torch.cat([mids, edges[-1:]]), torch.cat([edges[:1], mids])
                t = lower + (upper - lower) * T.rand_uniform(seed, 0, B, n0 + 1, ctx=c)
            else:
                t = edges[None, :].expand(B, n0 + 1).contiguous()
            d_enc = ops.pos_enc(viewdirs, 0, self.deg_view, ctx=c)
        out, used, kept = [], [], []
        for level, mlp in enumerate((self.coarse_mlp, self.fine_mlp)):
            N = t.shape[1]
            with torch.no_grad():
                keep, count, index, x_enc, cond = _train_rows(c, bits, G, lo, hi, clip, rays_o, viewdirs, t, d_enc)
                K = int(count.item()) if B else 0      # the one blocking read of this level
            kept.append(K)
            used.append((t, keep))
            raw_rgb, raw_sigma = nerf_mlp_rows(mlp, x_enc[:K], cond[:K], ctx=c)
            u_noise = T.rand_uniform(seed, 4 + 2 * level, B, N, ctx=c) if noise > 0.0 else None
            packed = scatter_activate(raw_rgb, raw_sigma, index[:K], B * N, u_noise, noise, ctx=c).reshape(B, N, 4)
            comp_rgb, acc, w, _, depth = T.composite(0, packed, None, t, rays_d, None, white_bkgd, ctx=c)
            out.append((comp_rgb, acc, depth))
            if level == 0:
                with torch.no_grad():
                    if randomized:
                        t = T.resample_u(t, w, T.rand_uniform(seed, 2, B, n1, ctx=c), False, ctx=c)
                    else:
                        t = ops.resample(t, w.detach(), n1, False, ctx=c)
        self.last_train_kept = tuple(kept)
        self._raise_flags(c.poll_flags())
        return (out, used) if return_samples else out

    @torch.no_grad()
    def _occupancy_sigma(self, box, resolution, probes, points_per_piece=1 << 22):
        """max(sigma of slot 0, sigma of slot 1) on the lattice of `occupancy_lattice_box`, its columns evaluated as rays by
        `eval_mlp` in pieces of at most points_per_piece points; the maximum is taken on the device."""
        dev = next(self.parameters()).device
        M = resolution * probes
        c, o, d = occupancy_lattice_box(box, resolution, probes, dev)
        sigma = torch.empty(M * M, M, device=dev)
        step = max(1, points_per_piece // M)
        for i in range(0, M * M, step):
            oo, dd = o[i:i + step], d[i:i + step]
            t = c[None, :].expand(oo.shape[0], M).contiguous()
            sigma[i:i + step] = torch.maximum(self.eval_mlp(0, oo, dd, t)[..., 3], self.eval_mlp(1, oo, dd, t)[..., 3])
        return sigma.reshape(M, M, M)

    @torch.no_grad()
    def build_occupancy(self, box, resolution, sigma_threshold, probes=2, dilate=1, clip=False):
        """Builds, installs and returns the grid of this module's scene over box = (lo, hi): both MLPs are evaluated on the
        (resolution * probes)^3 lattice of cell sub-centres (a vanilla density depends on the position alone), a cell is occupied
        iff the larger of the two densities at one of its probes is not <= sigma_threshold, and the result is dilated by `dilate`
        cells over the 26-neighbourhood, on the device (`occupancy_from_sigma_box`).  sigma_threshold has no default: nobody has
        measured one on trained weights (`models.NeRF_TP.build_occupancy` says how to read it as an opacity).  ValueError, before
        any device access, for a bad box, resolution, probes, dilate or threshold."""
        G, probes, dilate = ops._check_build(resolution, sigma_threshold, probes, dilate, "build_occupancy")
        box = _check_box(box, "build_occupancy")
        sigma = self._occupancy_sigma(box, G, probes)
        grid = occupancy_from_sigma_box(sigma, G, sigma_threshold, probes, dilate, ctx=self._context(sigma.device))
        self.set_occupancy(grid, box, clip)
        return grid

    @torch.no_grad()
    def render_marching(self, rays, eps, white_bkgd, near, far, segment=64, coarse=False, grid=True, return_samples=False):
        """`forward(rays, False, white_bkgd, near, far)` in which a sample is evaluated iff the installed grid keeps it
        (`occupancy_keep_box`; grid=False or no grid: every sample is kept) AND it lies in front of the ray's stop
        (neo_vanilla_render_marching).  The stop is `termination_stops_vanilla` on the level's rows with the samples that are not
        kept zeroed: segment 0 is always marched, segment k >= 1 iff the transmittance at every earlier boundary was not below
        eps.  A sample that is not evaluated has a zero row and weight exactly 0; an evaluated one is bitwise `eval_mlp`'s.
        Level 1 follows the stop rule; level 0 only with coarse=True, which moves the level-1 positions: NO bound is claimed for
        that mode.  With coarse=False, against the same call at eps = 0: a ray that never stops is bitwise equal, and a stopped
        ray's level-1 rgb differs by at most 1.003 * trans per channel and its depth by at most 1.001 * far * trans, trans < eps
        being its transmittance at the stop.  Without a grid and at eps = 0 the result is bitwise `forward`'s.
        ValueError, before any device access, for eps outside [0, 1) or NaN, or a segment that is not a positive multiple of 64;
        NeoError when grid=True and the installed grid belongs to another context.

        Returns [(rgb (B,3), acc (B,), depth (B,))] * 2; with return_samples a third element holds per level
        (t (B,N), weights (B,N), keep (B,N) bool - the grid's verdict on the whole row, behind the stop as well - stop (B,) int32,
        rows (B,N,4)): the evaluated set is keep & (j < stop).  `self.last_march_kept` (int64[2]: evaluated samples per level)
        stays on the device; nothing is read back."""
        eps, segment = ops._check_termination(eps, segment, "render_marching")
        raw = (rays["rays_o"], rays["viewdirs"], rays["rays_d"])
        rays_o, viewdirs, rays_d = ray_rows(rays, ("rays_o", "viewdirs", "rays_d"))
        dev = rays_o.device
        ctx = self._context(dev)
        if grid and self._occupancy is not None and self._occ_ctx is not ctx:
            raise _lib.NeoError("the occupancy grid does not belong to this module's context on %s: install it again" % dev)
        self._sync_weights(ctx)
        self._before_call(ctx)
        B = rays_o.shape[0]
        n = (self.num_coarse_samples + 1, self.num_coarse_samples + 1 + self.num_fine_samples)
        outs, samples, counts = [], [], []

        def launch():
            self._set_mode(ctx, "_vanilla_window", "neo_vanilla_set_march_window", int(self.march_window or 0))
            outs.extend((torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)) for _ in range(2))
            structs = [None, None]
            if return_samples:
                t0 = torch.empty(n[0], device=dev)
                for lv in range(2):
                    s = dict(t=t0 if lv == 0 else torch.empty(B, n[1], device=dev), w=torch.empty(B, n[lv], device=dev),
                             keep=torch.empty(B, n[lv], dtype=torch.bool, device=dev),
                             stop=torch.empty(B, dtype=torch.int32, device=dev), rows=torch.empty(B, n[lv], 4, device=dev))
                    samples.append(s)
                    structs[lv] = ctypes.byref(_lib.VanillaMarchSamples(*(s[k].data_ptr() for k, _ in _lib.VanillaMarchSamples._fields_)))
            counts.append(torch.empty(2, dtype=torch.int64, device=dev))
            _lib.check(ctx.lib.neo_vanilla_render_marching(
                ctx.handle, ptr(rays_o), ptr(viewdirs), ptr(rays_d), B, float(near), float(far), self.num_coarse_samples,
                self.num_fine_samples, int(bool(white_bkgd)), eps, segment, int(bool(coarse)), int(bool(grid)),
                ptr(outs[0][0]), ptr(outs[0][1]), ptr(outs[0][2]), ptr(outs[1][0]), ptr(outs[1][1]), ptr(outs[1][2]),
                structs[0], structs[1], counts[0].data_ptr(), ctx.stream()))
            self._after_call(ctx)
            return [t for lv in outs for t in lv] + [v for s in samples for v in s.values()] + counts
        self._launch_overlapped(ctx, dev, raw, (rays_o, viewdirs, rays_d), launch)
        self.last_march_kept = counts[0]
        out = list(outs)
        if return_samples:
            samples[0]["t"] = samples[0]["t"][None, :].expand(B, n[0])
            out.append([tuple(s[k] for k in ("t", "w", "keep", "stop", "rows")) for s in samples])
        return out


_PIX_SRC_KEYS = ("src_poses", "src_focal", "src_c", "src_imgs")


class MarchingPixelNeRF(_BoxOccupancy, models.PixelNeRF):
    """`models.PixelNeRF` - same constructor, `state_dict` keys, `forward`, `eval_mlp` and training path - with an occupancy grid
    over a box and the marching frame (include/neo360_hip.h: PIXELNERF MARCHING FRAME).  Given the scene latent, the source cameras
    and the weights, a PixelNeRF density depends on the position alone, so the grid describes ONE scene: `set_scene` removes it."""

    # rays per window of render_marching (None: the library's default); results do not depend on it
    march_window = None
    _occ_entry = "neo_pix_set_occupancy"

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._init_box_occupancy()

    @torch.no_grad()
    def set_scene(self, latent, image_wh):
        """`PixelNeRF.set_scene`, after which no grid is installed: a grid describes one scene (as `NeRF_TP.set_scene`).  An
        attached encoder that runs again on new `src_imgs` therefore falls back to "no grid" - slower, never wrong."""
        super().set_scene(latent, image_wh)
        self.set_occupancy(None)

    @torch.no_grad()
    def _occupancy_sigma(self, rays, box, resolution, probes, points_per_piece=1 << 20):
        """max(sigma of slot 0, sigma of slot 1) on the lattice of `occupancy_lattice_box`, its columns evaluated as rays by
        `eval_mlp` in pieces of at most points_per_piece points; the maximum is taken on the device."""
        dev = next(self.parameters()).device
        M = resolution * probes
        c, o, d = occupancy_lattice_box(box, resolution, probes, dev)
        src = {k: rays[k] for k in _PIX_SRC_KEYS if k in rays}
        sigma = torch.empty(M * M, M, device=dev)
        step = max(1, points_per_piece // M)
        for i in range(0, M * M, step):
            piece = dict(src, rays_o=o[i:i + step], rays_d=d[i:i + step], viewdirs=d[i:i + step])
            t = c[None, :].expand(piece["rays_o"].shape[0], M).contiguous()
            sigma[i:i + step] = torch.maximum(self.eval_mlp(0, piece, t)[..., 3], self.eval_mlp(1, piece, t)[..., 3])
        return sigma.reshape(M, M, M)

    @torch.no_grad()
    def build_occupancy(self, rays, box, resolution, sigma_threshold, probes=2, dilate=1, clip=False):
        """Builds, installs and returns the grid of the current scene over box = (lo, hi).  rays supplies the source cameras
        (`src_poses`, `src_focal`, `src_c`; `src_imgs` for an attached encoder) - its own rays are not read.  Both MLPs are
        evaluated with `eval_mlp` on the (resolution * probes)^3 lattice of cell sub-centres, a cell is occupied iff the larger of
        the two densities at one of its probes is not <= sigma_threshold, and the result is dilated by `dilate` cells over the
        26-neighbourhood, on the device (`occupancy_from_sigma_box`).  sigma_threshold has no default: nobody has measured one on
        trained weights.  ValueError, before any device access, for a bad box, resolution, probes, dilate or threshold."""
        G, probes, dilate = ops._check_build(resolution, sigma_threshold, probes, dilate, "build_occupancy")
        box = _check_box(box, "build_occupancy")
        sigma = self._occupancy_sigma(rays, box, G, probes)
        grid = occupancy_from_sigma_box(sigma, G, sigma_threshold, probes, dilate, ctx=self._context(sigma.device))
        self.set_occupancy(grid, box, clip)
        return grid

    @torch.no_grad()
    def render_marching(self, rays, eps, white_bkgd, near, far, chunk=None, segment=64, coarse=False, grid=True, return_samples=False):
        """`forward(rays, False, white_bkgd, near, far, chunk)` in which a sample is evaluated iff the installed grid keeps it
        (`occupancy_keep_box` with dirs = rays_d; grid=False or no grid: every sample is kept) AND it lies in front of its ray's
        stop (neo_pix_render_marching).  The stop is `termination_stops_vanilla` on the level's rows with the samples that are not
        kept zeroed: segment 0 is always marched, segment k >= 1 iff the transmittance at every earlier boundary was not below
        eps.  A sample that is not evaluated has a zero row and weight exactly 0; an evaluated one is bitwise `eval_mlp`'s at the
        call's `chunk` (all rays of the call form ONE reference chunk unless chunk is given: the direction a sample is seen along
        is that of ray (b N + j) mod B of its chunk, as in `forward`).
        Level 1 follows the stop rule; level 0 only with coarse=True, which moves the level-1 positions: NO bound is claimed for
        that mode.  With coarse=False, against the same call at eps = 0: a ray that never stops is bitwise equal, and a stopped
        ray's level-1 rgb differs by at most 1.003 * trans per channel and its depth by at most 1.001 * far * trans, trans < eps
        being its transmittance at the stop.  Without a grid at eps = 0, with grid=False, with an all-ones grid, or with a box that
        holds no sample and clip=False, the six outputs are bitwise `forward`'s.  Results do not depend on `march_window`, on the
        stream, or on whether a frame is one call or the caller's loop over its reference chunks.
        ValueError, before any device access, for eps outside [0, 1) or NaN, a segment that is not a positive multiple of 64, or
        a chunk that is not a positive integer; NeoError when grid=True and the installed grid belongs to another context.

        Returns [(rgb (B,3), acc (B,), depth (B,))] * 2; with return_samples a third element holds per level
        (t (B,N), weights (B,N), keep (B,N) bool - the grid's verdict on the whole row, behind the stop as well - stop (B,) int32,
        rows (B,N,4)): the evaluated set is keep & (j < stop).  `self.last_march_kept` (int64[2]: evaluated samples per level)
        stays on the device; nothing is read back."""
        eps, segment = ops._check_termination(eps, segment, "render_marching")
        if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1):
            raise ValueError("render_marching: chunk must be a positive integer or None, got %r" % (chunk,))
        raw = (rays["rays_o"], rays["rays_d"], rays["viewdirs"])
        rays_o, rays_d, viewdirs = ray_rows(rays)
        dev = rays_o.device
        ctx = self._context(dev)
        self._ensure_scene(rays)       # an encoder that runs again removes the grid (set_scene)
        if self._scene_ctx is not ctx:
            raise _lib.NeoError("the scene latent was uploaded on a different device")
        if grid and self._occupancy is not None and self._occ_ctx is not ctx:
            raise _lib.NeoError("the occupancy grid does not belong to this module's context on %s: install it again" % dev)
        self._sync_weights(ctx)
        self._before_call(ctx)
        B = rays_o.shape[0]
        host_poses, NV, focal, cx, cy = self._camera_args(rays)
        n = (self.num_coarse_samples + 1, self.num_coarse_samples + 1 + self.num_fine_samples)
        outs, samples, counts = [], [], []

        def launch():
            self._set_mode(ctx, "_pix_window", "neo_pix_set_march_window", int(self.march_window or 0))
            outs.extend((torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)) for _ in range(2))
            structs = [None, None]
            if return_samples:
                t0 = torch.empty(n[0], device=dev)
                for lv in range(2):
                    s = dict(t=t0 if lv == 0 else torch.empty(B, n[1], device=dev), w=torch.empty(B, n[lv], device=dev),
                             keep=torch.empty(B, n[lv], dtype=torch.bool, device=dev),
                             stop=torch.empty(B, dtype=torch.int32, device=dev), rows=torch.empty(B, n[lv], 4, device=dev))
                    samples.append(s)
                    structs[lv] = ctypes.byref(_lib.VanillaMarchSamples(*(s[k].data_ptr() for k, _ in _lib.VanillaMarchSamples._fields_)))
            counts.append(torch.empty(2, dtype=torch.int64, device=dev))
            _lib.check(ctx.lib.neo_pix_render_marching(
                ctx.handle, ptr(rays_o), ptr(rays_d), ptr(viewdirs), B, int(chunk or max(B, 1)), host_poses, NV, focal, cx, cy,
                float(near), float(far), self.num_coarse_samples, self.num_fine_samples, int(bool(white_bkgd)), eps, segment,
                int(bool(coarse)), int(bool(grid)), ptr(outs[0][0]), ptr(outs[0][1]), ptr(outs[0][2]), ptr(outs[1][0]),
                ptr(outs[1][1]), ptr(outs[1][2]), structs[0], structs[1], counts[0].data_ptr(), ctx.stream()))
            self._after_call(ctx)
            return [t for lv in outs for t in lv] + [v for s in samples for v in s.values()] + counts
        self._launch_overlapped(ctx, dev, raw, (rays_o, rays_d, viewdirs), launch)
        self.last_march_kept = counts[0]
        out = list(outs)
        if return_samples:
            samples[0]["t"] = samples[0]["t"][None, :].expand(B, n[0])
            out.append([tuple(s[k] for k in ("t", "w", "keep", "stop", "rows")) for s in samples])
        return out


@torch.no_grad()
def render_marching_rays(model, batch, eps, chunk=32768, white_bkgd=False, near=0.2, far=3.0, segment=64, coarse=False, grid=True,
                         check=True, on_range="retry_f32"):
    """Frame of a MarchingNeRF or a MarchingPixelNeRF with empty space skipped and early ray termination: the fine level of
    `model.render_marching(batch, eps, ...)` on every ray of `batch`.  MarchingNeRF: `chunk` rays a library call (a vanilla ray does
    not depend on its chunk: the chunk only bounds the workspace).  MarchingPixelNeRF: ONE library call per frame with the reference
    `chunk` passed down, as `render.render_rays_test` does for PixelNeRF - a PixelNeRF ray depends on its chunk - and `batch` carries
    the source cameras.  Returns dict(rgb (R,3), depth (R,), acc (R,)) plus `kept_fraction`, a (2,) float64 DEVICE tensor - the
    share of samples evaluated at level 0 and level 1 (reading it synchronises, the call does not) - and `target` /
    `instance_mask` passed through.  check / on_range: the flag read, range-guard retry and latch of `render.render_rays_test` (the
    same code path); a retry lands on the compact instantiation of the exact kernel."""
    from . import render
    if not isinstance(model, (MarchingNeRF, MarchingPixelNeRF)):
        raise TypeError("render_marching_rays renders MarchingNeRF and MarchingPixelNeRF modules, got %r" % type(model))
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError("render_marching_rays: chunk must be a positive integer, got %r" % (chunk,))
    ops._check_termination(eps, segment, "render_marching_rays")
    pix = isinstance(model, MarchingPixelNeRF)
    rays_o, viewdirs, rays_d = ray_rows(batch, ("rays_o", "viewdirs", "rays_d"), on_device=False)
    R = rays_o.shape[0]
    n0 = model.num_coarse_samples + 1
    per = (float(max(R * n0, 1)), float(max(R * (n0 + model.num_fine_samples), 1)))      # scalar divisors: no host read, no copy

    def once():
        parts, kept = [], None
        if pix:
            frame = dict({k: batch[k] for k in _PIX_SRC_KEYS if k in batch}, rays_o=rays_o, viewdirs=viewdirs, rays_d=rays_d)
            parts.append(model.render_marching(frame, eps, white_bkgd, near, far, chunk=chunk, segment=segment, coarse=coarse,
                                               grid=grid)[1])
            kept = model.last_march_kept
        else:
            for i in range(0, max(R, 1), chunk):
                part = dict(rays_o=rays_o[i:i + chunk], viewdirs=viewdirs[i:i + chunk], rays_d=rays_d[i:i + chunk])
                parts.append(model.render_marching(part, eps, white_bkgd, near, far, segment=segment, coarse=coarse, grid=grid)[1])
                kept = model.last_march_kept if kept is None else kept + model.last_march_kept
        kept = kept.double()
        return dict(rgb=torch.cat([p[0] for p in parts]), acc=torch.cat([p[1] for p in parts]), depth=torch.cat([p[2] for p in parts]),
                    kept_fraction=torch.stack([kept[0] / per[0], kept[1] / per[1]]))
    return render._render_guarded(model, batch, once, check, on_range)
