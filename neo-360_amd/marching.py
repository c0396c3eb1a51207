"""Empty-space skipping and early ray termination for the vanilla renderer (include/neo360_hip.h: VANILLA MARCHING FRAME).

`MarchingNeRF` is `models.NeRF` - same constructor, `state_dict` keys and `forward` - with an occupancy grid over a caller-given
box and `render_marching`, the frame in which a sample is evaluated iff the grid keeps it AND it lies in front of the ray's stop.
The stage functions expose the rules the frame is made of, on caller rows:

    occupancy_keep_box          the BOX KEEP RULE (neo_vanilla_occupancy_keep)
    occupancy_from_sigma_box    a lattice of densities -> a grid, no unit-sphere clip (neo_occupancy_from_sigma_box)
    termination_stops_vanilla   the MODE-0 STOP RULE (neo_vanilla_termination_stops)
    eval_points                 the compact evaluator launch: single points under a device count (neo_vanilla_mlp_compact)
    render_marching_rays        the frame helper

Every caller tensor goes through `context.dense` / `context.owned_output`; a bad shape, dtype, G, box, eps or segment raises
ValueError before any device access.
"""
import ctypes
import math

import torch

from . import _lib, models, ops
from .context import dense, owned_output, ptr, ray_rows


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


class MarchingNeRF(models.NeRF):
    """`models.NeRF` with an occupancy grid over a box and the marching frame.  `forward`, `eval_mlp` and the training path are
    the parent's and read none of this."""

    # rays per window of render_marching (None: the library's default, 8192): a window bounds the extra workspace at 68 bytes per
    # (ray, sample) of one window and segment; results do not depend on it
    march_window = None

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._occupancy = self._occ_box = self._occ_ctx = None
        self._occ_clip = False
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
                _lib.check(c.lib.neo_vanilla_set_occupancy(c.handle, None, 0, None, None, 0, c.stream()))
            self._occupancy = self._occ_box = self._occ_ctx = None
            self._occ_clip = False
            return
        G = ops._check_occupancy(grid, "set_occupancy")
        lo, hi = _check_box(box, "set_occupancy")
        dev = next(self.parameters()).device
        ctx = self._context(dev)
        occ = grid.detach().to(dev).contiguous().clone()
        bits = ops.pack_occupancy(occ)
        _lib.check(ctx.lib.neo_vanilla_set_occupancy(ctx.handle, ptr(bits), G, _c3(lo), _c3(hi), int(bool(clip)), ctx.stream()))
        self._occupancy, self._occ_box, self._occ_clip, self._occ_ctx = occ, (lo, hi), bool(clip), ctx

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


@torch.no_grad()
def render_marching_rays(model, batch, eps, chunk=32768, white_bkgd=False, near=0.2, far=3.0, segment=64, coarse=False, grid=True,
                         check=True, on_range="retry_f32"):
    """Frame of a MarchingNeRF with empty space skipped and early ray termination: the fine level of
    `model.render_marching(batch, eps, ...)` on every ray of `batch`, `chunk` rays a library call (a vanilla ray does not depend on
    its chunk: the chunk only bounds the workspace).  Returns dict(rgb (R,3), depth (R,), acc (R,)) plus `kept_fraction`, a (2,)
    float64 DEVICE tensor - the share of samples evaluated at level 0 and level 1 (reading it synchronises, the call does not) -
    and `target` / `instance_mask` passed through.  check / on_range: the flag read, range-guard retry and latch of
    `render.render_rays_test` (the same code path)."""
    from . import render
    if not isinstance(model, MarchingNeRF):
        raise TypeError("render_marching_rays renders MarchingNeRF modules, got %r" % type(model))
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError("render_marching_rays: chunk must be a positive integer, got %r" % (chunk,))
    ops._check_termination(eps, segment, "render_marching_rays")
    rays_o, viewdirs, rays_d = ray_rows(batch, ("rays_o", "viewdirs", "rays_d"), on_device=False)
    R = rays_o.shape[0]

    def once():
        parts, kept = [], None
        for i in range(0, max(R, 1), chunk):
            part = dict(rays_o=rays_o[i:i + chunk], viewdirs=viewdirs[i:i + chunk], rays_d=rays_d[i:i + chunk])
            parts.append(model.render_marching(part, eps, white_bkgd, near, far, segment=segment, coarse=coarse, grid=grid)[1])
            kept = model.last_march_kept if kept is None else kept + model.last_march_kept
        n0 = model.num_coarse_samples + 1
        per = (float(max(R * n0, 1)), float(max(R * (n0 + model.num_fine_samples), 1)))      # scalar divisors: no host read, no copy
        kept = kept.double()
        return dict(rgb=torch.cat([p[0] for p in parts]), acc=torch.cat([p[1] for p in parts]), depth=torch.cat([p[2] for p in parts]),
                    kept_fraction=torch.stack([kept[0] / per[0], kept[1] / per[1]]))
    return render._render_guarded(model, batch, once, check, on_range)
