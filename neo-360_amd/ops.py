"""Stage-level operators over the C ABI — the GPU counterparts of the reference's
helper functions, used by the modules in `models.py` and by the stage-isolated
parity tests.  Inputs and outputs are PyTorch-ROCm tensors."""
import ctypes

import torch

from . import _lib
from .context import dense, f32, f64, get_context, owned_output, ptr


def _ctx(t, ctx):
    return ctx if ctx is not None else get_context(t.device)


def get_ray_directions_and_rays(H, W, focal, c2w, ctx=None, device="cuda", ray_range=None, out=None):
    """datasets/ray_utils.py:84-104 + :133-176 in one kernel.
    c2w: (3,4) or (4,4) array-like (host).  Returns rays_o, viewdirs, rays_d (n,3), radii (n,) for the whole frame
    (n = H W) or for rays [lo, hi) of it when ray_range = (lo, hi) (a rank's shard).  `out`: the four tensors to write into
    (e.g. the previous frame's, so a render loop allocates nothing): dense, 16-byte-aligned fp32 tensors of exactly these
    shapes on the context's device - anything else is refused (ValueError / TypeError), nothing is written through a copy."""
    ctx = ctx if ctx is not None else get_context(device)
    dev = ctx.device
    pose = torch.as_tensor(c2w, dtype=torch.float32, device="cpu")[:3, :4].contiguous()
    host = (ctypes.c_float * 12)(*pose.reshape(-1).tolist())
    lo, hi = ray_range if ray_range is not None else (0, H * W)
    n = hi - lo
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 4:
            raise ValueError("out must be the four tensors (rays_o, viewdirs, rays_d, radii)")
        rays_o, viewdirs, rays_d, radii = (owned_output(t, "out[%d] (%s)" % (i, k), sh, device=dev) for i, (t, k, sh) in enumerate(
            zip(out, ("rays_o", "viewdirs", "rays_d", "radii"), ((n, 3), (n, 3), (n, 3), (n,)))))
        _lib.note_external_write()      # same tensor objects, same version counters, new contents
    else:
        rays_o = torch.empty(n, 3, device=dev)
        viewdirs = torch.empty(n, 3, device=dev)
        rays_d = torch.empty(n, 3, device=dev)
        radii = torch.empty(n, device=dev)
    _lib.check(ctx.lib.neo_raygen_range(ctx.handle, H, W, float(focal), host, int(lo), int(n), ptr(rays_o), ptr(viewdirs),
                                        ptr(rays_d), ptr(radii), ctx.stream()))
    return rays_o, viewdirs, rays_d, radii


def _ray_pair(a, name_a, b, name_b, to=torch.float32):
    """Two (R,3) ray tensors of one call: `a` defines R and the device, `b` must match it."""
    a = dense(a, name_a, (None, 3), to=to)
    return a, dense(b, name_b, (a.shape[0], 3), to=to, device=a.device)


def bbox_intersection_batch(bounds, rays_o, rays_d, ctx=None):
    """datasets/ray_utils.py:17-31 (float64).  bounds (2,3) host array-like; rays in the
    box frame, (R,3) device tensors (rays_o defines R; any float dtype and any strides, read as float64).  Returns hit (uint8), tmin, tmax (float64)."""
    rays_o, rays_d = _ray_pair(rays_o, "rays_o", rays_d, "rays_d", torch.float64)
    ctx = _ctx(rays_o, ctx)
    R = rays_o.shape[0]
    b = torch.as_tensor(bounds, dtype=torch.float64, device="cpu").reshape(6)
    host = (ctypes.c_double * 6)(*b.tolist())
    hit = torch.empty(R, dtype=torch.uint8, device=rays_o.device)
    tmin = torch.empty(R, dtype=torch.float64, device=rays_o.device)
    tmax = torch.empty(R, dtype=torch.float64, device=rays_o.device)
    _lib.check(ctx.lib.neo_aabb_intersect(ctx.handle, host, ptr(rays_o), ptr(rays_d), R, ptr(hit), ptr(tmin),
                                          ptr(tmax), ctx.stream()))
    return hit, tmin, tmax


def _box_tables(RTs):
    """Host tables of the boxes of an `RTs` dict: (n, 16 n doubles of world -> box frames, 6 n doubles of bounds)."""
    import numpy as np
    mats, bounds = [], []
    for rot, tran, sca in zip(RTs["R"], RTs["T"], RTs["s"]):
        box = np.eye(4)                                         # helper.py:352-356, verbatim order of operations
        box[:3, :3] = np.reshape(np.array(rot), (3, 3))
        box[:3, -1] = np.array(tran)
        mats.append(np.linalg.inv(box))
        bounds.append(np.asarray(sca, dtype=np.float64).reshape(6))
    n = len(mats)
    if n == 0:
        return 0, None, None
    hm = (ctypes.c_double * (16 * n))(*np.stack(mats).astype(np.float64).reshape(-1).tolist())
    hb = (ctypes.c_double * (6 * n))(*np.stack(bounds).reshape(-1).tolist())
    return n, hm, hb


def sample_rays_in_bbox(RTs, rays_o, view_dirs, ctx=None, return_per_box=False):
    """models/neo360/helper.py:359-373 (with get_object_rays_in_bbox :348-357 and get_rays_in_bbox :333-346 inside):
    RTs = dict(R=[3x3 or 9], T=[3], s=[(2,3) bounds]) per object; rays are moved into every box frame in float64,
    slab-tested, and merged with 0 as the "no hit" sentinel.  rays_o / view_dirs: (R,3) device tensors (rays_o defines R; any
    strides, any float dtype; the reference's NumPy arrays are promoted to float64 the same way).  Returns all_near (R,1), all_far (R,1)
    float32 and bbox_mask (R,1) bool, as the reference; with return_per_box also the per-box hit masks (n,R)."""
    rays_o, view_dirs = _ray_pair(rays_o, "rays_o", view_dirs, "view_dirs", torch.float64)
    ctx = _ctx(rays_o, ctx)
    R = rays_o.shape[0]
    n, hm, hb = _box_tables(RTs)
    dev = rays_o.device
    if n == 0:
        # a scene without objects: the reference's loops never run and its zero-initialised outputs come back
        # (helper.py:359-373): near = far = 0, mask all False
        zero = torch.zeros(R, 1, device=dev)
        mask = torch.zeros(R, 1, dtype=torch.bool, device=dev)
        if return_per_box:
            return zero, zero.clone(), mask, torch.empty(0, R, dtype=torch.uint8, device=dev)
        return zero, zero.clone(), mask
    near = torch.empty(R, 1, device=dev)
    far = torch.empty(R, 1, device=dev)
    mask = torch.empty(R, 1, dtype=torch.uint8, device=dev)
    per_box = torch.empty(n, R, dtype=torch.uint8, device=dev) if return_per_box else None
    _lib.check(ctx.lib.neo_aabb_multi(ctx.handle, n, hm, hb, ptr(rays_o), ptr(view_dirs), R, ptr(per_box), ptr(near),
                                      ptr(far), ptr(mask), ctx.stream()))
    if return_per_box:
        return near, far, mask.bool(), per_box
    return near, far, mask.bool()


def sample_rays_in_bbox_list(RTs, rays_o, view_dirs, ctx=None):
    """models/neo360/helper.py:375-394: the interval of EVERY box instead of the merged one (which keeps the smallest near and
    the smallest far over the boxes a ray meets, so a ray that clips a front box never reaches the object behind it).  Inputs as
    sample_rays_in_bbox, the same float64 transform and slab test.  Returns all_near (K,R,1), all_far (K,R,1) float32 with the
    reference's 0 = "no hit" sentinel (its stacked shape) and hit (K,R) bool - the reference's third value is a leftover of its
    loop, ours is the mask.  K = 0 returns empty tensors.  What `NeRF_TP.render_instances` takes as near_inst / far_inst."""
    rays_o, view_dirs = _ray_pair(rays_o, "rays_o", view_dirs, "view_dirs", torch.float64)
    ctx = _ctx(rays_o, ctx)
    R = rays_o.shape[0]
    n, hm, hb = _box_tables(RTs)
    dev = rays_o.device
    near = torch.empty(n, R, 1, device=dev)
    far = torch.empty(n, R, 1, device=dev)
    hit = torch.empty(n, R, dtype=torch.uint8, device=dev)
    if n:
        _lib.check(ctx.lib.neo_aabb_per_box(ctx.handle, n, hm, hb, ptr(rays_o), ptr(view_dirs), R, ptr(near), ptr(far), ptr(hit),
                                            ctx.stream()))
    return near, far, hit.bool()


def intersect_sphere(rays_o, rays_d, ctx=None, check=True):
    """models/neo360/helper.py:253-273.  rays_o (R,3) defines R, rays_d (R,3); any float dtype, any strides.  Returns far (R,1) and the per-ray hit mask (uint8).
    Raises AssertionError like the reference when a ray misses the unit sphere."""
    rays_o, rays_d = _ray_pair(rays_o, "rays_o", rays_d, "rays_d")
    ctx = _ctx(rays_o, ctx)
    R = rays_o.shape[0]
    far = torch.empty(R, 1, device=rays_o.device)
    ok = torch.empty(R, dtype=torch.uint8, device=rays_o.device)
    _lib.check(ctx.lib.neo_intersect_sphere(ctx.handle, ptr(rays_o), ptr(rays_d), R, ptr(far), ptr(ok), ctx.stream()))
    if check and (ctx.poll_flags() & 1):
        raise AssertionError("1.0 - p_norm_sq should be greater than 0")
    return far, ok


def pos_enc(x, min_deg, max_deg, ctx=None):
    """neo360/helper.py:121-125 == vanilla_nerf/helper.py:445-449.  x (..., C), any float dtype, any strides."""
    if isinstance(x, torch.Tensor) and x.dim() < 1:
        raise ValueError("x must have shape (..., C), got %s" % (tuple(x.shape),))
    x = dense(x, "x")
    ctx = _ctx(x, ctx)
    C = x.shape[-1]
    n = x.numel() // C
    out = torch.empty(*x.shape[:-1], C * (2 * (max_deg - min_deg) + 1), device=x.device)
    _lib.check(ctx.lib.neo_pos_enc(ctx.handle, ptr(x), n, C, min_deg, max_deg, ptr(out), ctx.stream()))
    return out


def resample(t_prev, weights, n_new, descending=False, ctx=None):
    """sorted_piecewise_constant_pdf + the sort of sample_pdf, with the callers'
    slicing (bins = midpoints of t_prev, pdf weights = weights[:,1:-1]).  t_prev (R,n) defines R and n, weights (R,n);
    any float dtype, any strides.  Returns (R, n + n_new)."""
    t_prev = dense(t_prev, "t_prev", (None, None))
    R, n_prev = t_prev.shape
    weights = dense(weights, "weights", (R, n_prev), device=t_prev.device)
    ctx = _ctx(t_prev, ctx)
    out = torch.empty(R, n_prev + n_new, device=t_prev.device)
    _lib.check(ctx.lib.neo_resample(ctx.handle, ptr(t_prev), ptr(weights), R, n_prev, n_new, int(descending),
                                    ptr(out), ctx.stream()))
    return out


def _composite_args(mode, rgbsigma, t, rays_d, t_far):
    """The tensor contract of neo_composite, shared with training.composite: t (R,N) defines R, N and the device; rgbsigma
    (R,N,4); rays_d (R,3), read by modes 0 and 1 and required there; t_far (R,) or (R,1), read by mode 1 and required there.
    What a mode does not read is still checked when given; a missing one is the library's error (NeoError), as before."""
    t = dense(t, "t", (None, None))
    R, N = t.shape
    rgbsigma = dense(rgbsigma, "rgbsigma", (R, N, 4), device=t.device)
    rays_d = dense(rays_d, "rays_d", (R, 3), device=t.device) if rays_d is not None else None
    t_far = dense(t_far, "t_far", [(R,), (R, 1)], device=t.device) if t_far is not None else None
    return rgbsigma, t, rays_d, t_far


def composite(mode, rgbsigma, t, rays_d=None, t_far=None, white_bkgd=False, ctx=None):
    """volumetric_rendering; mode 0 vanilla, 1 NeO-360 inside, 2 NeO-360 outside.  t (R,N) defines R and N; rgbsigma (R,N,4),
    rays_d (R,3) (modes 0, 1), t_far (R,) or (R,1) (mode 1); any float dtype, any strides.
    Returns dict(rgb, acc, depth, weights, bg_lambda)."""
    rgbsigma, t, rays_d, t_far = _composite_args(mode, rgbsigma, t, rays_d, t_far)
    ctx = _ctx(t, ctx)
    R, N = t.shape
    dev = t.device
    rgb = torch.empty(R, 3, device=dev)
    acc = torch.empty(R, device=dev)
    depth = torch.empty(R, device=dev)
    w = torch.empty(R, N, device=dev)
    lam = torch.empty(R, 1, device=dev) if mode == 1 else None
    _lib.check(ctx.lib.neo_composite(ctx.handle, mode, ptr(rgbsigma), ptr(t), ptr(rays_d), ptr(t_far), R, N,
                                     int(bool(white_bkgd)), ptr(rgb), ptr(acc), ptr(depth), ptr(w), ptr(lam),
                                     ctx.stream()))
    return dict(rgb=rgb, acc=acc, depth=depth, weights=w, bg_lambda=lam)


def mip_resample(s_prev, w_prev, n, near, far, dilate=False, dilation=0.0, anneal=1.0, ctx=None):
    """One Mip-NeRF 360 proposal-resampling step (mipnerf360/model.py:258-310).  w_prev (R,n_prev) defines R and n_prev,
    s_prev (R,n_prev+1); any float dtype, any strides.  Returns sdist, tdist (R,n+1)."""
    w_prev = dense(w_prev, "w_prev", (None, None))
    R, n_prev = w_prev.shape
    s_prev = dense(s_prev, "s_prev", (R, n_prev + 1), device=w_prev.device)
    ctx = _ctx(s_prev, ctx)
    sdist = torch.empty(R, n + 1, device=s_prev.device)
    tdist = torch.empty(R, n + 1, device=s_prev.device)
    _lib.check(ctx.lib.neo_mip_resample(ctx.handle, ptr(s_prev), ptr(w_prev), R, n_prev, int(bool(dilate)),
                                        float(dilation), float(anneal), n, float(near), float(far), ptr(sdist),
                                        ptr(tdist), ctx.stream()))
    return sdist, tdist


def mip_composite(rgbdens, tdist, rays_d, bg=1.0, ctx=None):
    """compute_alpha_weights(opaque_background=True) + volumetric_rendering (mipnerf360/helper.py:246-274).
    tdist (R,n+1) defines R and n, rgbdens (R,n,4), rays_d (R,3); any float dtype, any strides.  Returns weights (R,n), rgb (R,3)."""
    tdist = dense(tdist, "tdist", (None, None))
    R, n1 = tdist.shape
    if n1 < 1:
        raise ValueError("tdist must have shape (R, n + 1), got %s" % (tuple(tdist.shape),))
    rgbdens = dense(rgbdens, "rgbdens", (R, n1 - 1, 4), device=tdist.device)
    rays_d = dense(rays_d, "rays_d", (R, 3), device=tdist.device)
    ctx = _ctx(tdist, ctx)
    w = torch.empty(R, n1 - 1, device=tdist.device)
    rgb = torch.empty(R, 3, device=tdist.device)
    _lib.check(ctx.lib.neo_mip_composite(ctx.handle, ptr(rgbdens), ptr(tdist), ptr(rays_d), R, n1 - 1, float(bg), ptr(w),
                                         ptr(rgb), ctx.stream()))
    return w, rgb


_QUANTILES = {}     # (device, quantiles) -> the fp32 device table neo_mip_extras reads


def _quantile_table(u, dev):
    if isinstance(u, torch.Tensor):
        return dense(u.reshape(-1), "u", device=dev)
    key = (dev, tuple(float(x) for x in u))
    tab = _QUANTILES.get(key)
    if tab is None:
        tab = _QUANTILES[key] = torch.tensor(key[1], dtype=torch.float32, device=dev).reshape(-1)
    return tab


@torch.no_grad()
def mip_extras(edges, w, u=(0.05, 0.5, 0.95), near=0.0, far=0.0, ctx=None):
    """The extras volumetric_rendering leaves behind `compute_extras` (mipnerf360/helper.py:264-274) for an interval histogram:
    edges (..., n+1) non-decreasing, w (..., n) non-negative -> acc (...,) = sum w, distance_mean (...,) = the expected distance
    clipped to [t_0, t_n] (t_n on a row without weight) and percentiles (..., len(u)) = sorted_interp(u, integrate_weights(w), t)
    (helper.py:196-222).  near == far == 0: edges are metric distances; otherwise edges are sdist and t = s_to_t(edges) for that near /
    far, formed inside the kernel.  u: up to 8 ascending quantiles in [0, 1], a sequence (its device table is kept) or an fp32 device
    tensor.  No gradients: training.mip_expected_distance is the differentiable (acc, distance_mean)."""
    edges, w = dense(edges, "edges"), dense(w, "w")
    if edges.dim() < 1 or w.dim() < 1:
        raise ValueError("edges must have shape (..., n + 1) and w (..., n), got %s %s" % (tuple(edges.shape), tuple(w.shape)))
    n = w.shape[-1]
    if edges.shape[-1] != n + 1 or edges.shape[:-1] != w.shape[:-1]:
        raise ValueError("edges must hold one more entry per row than w, got %s %s" % (tuple(edges.shape), tuple(w.shape)))
    if edges.device != w.device:
        raise ValueError("edges must be on %s, got %s" % (w.device, edges.device))
    ctx = _ctx(w, ctx)
    e2, w2 = edges.reshape(-1, n + 1), w.reshape(-1, n)
    R, dev = w2.shape[0], w.device
    tab = _quantile_table(u, dev)
    n_u = tab.numel()
    acc, mean, pct = torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(R, n_u, device=dev)
    _lib.check(ctx.lib.neo_mip_extras(ctx.handle, ptr(e2), ptr(w2), R, n, float(near), float(far), ptr(tab), n_u, ptr(acc), ptr(mean),
                                      ptr(pct), ctx.stream()))
    lead = w.shape[:-1]
    return acc.reshape(lead), mean.reshape(lead), pct.reshape(*lead, n_u)


MAX_EXTRA_QUANTILES = 8


def _extras_row(t, name, shapes, dev):
    if not isinstance(t, torch.Tensor) or not t.is_floating_point():
        raise ValueError("%s must be a floating-point tensor, got %r" % (name, t.dtype if isinstance(t, torch.Tensor) else type(t).__name__))
    if tuple(t.shape) not in shapes:
        raise ValueError("%s must have shape %s, got %s" % (name, " or ".join(str(s) for s in shapes), tuple(t.shape)))
    if t.device != dev:
        raise ValueError("%s must be on the device of fg_t (%s), got %s" % (name, dev, t.device))
    return f32(t, name)


@torch.no_grad()
def tp_extras(fg_t, fg_w, far, rays_o, rays_d, bg_s=None, bg_w=None, bg_lambda=None, quantiles=(0.05, 0.5, 0.95), ctx=None):
    """Opacity, expected disparity and distance percentiles of a NeO-360 ray's WHOLE interval histogram, inside and outside the unit
    sphere together (neo_tp_extras).  Distances are in the unit of the ray parameter t of o + t d - the unit of the reference's
    fg_depth, not that of its comp_depth (neo360/model.py:523 adds a disparity to a distance).

    fg_t (R,N) ascending, fg_w (R,N), far (R,) or (R,1) the sphere exit (ops.intersect_sphere); rays_o, rays_d (R,3); bg_s (R,N)
    descending inverse radius, bg_w (R,N), bg_lambda (R,) or (R,1) the inside composite's last transmittance.  Without the three
    outside arguments: the inside-only histogram of N intervals ending at `far` (the rows of render_objects(return_samples=True)
    with far = far_obj).  M = 2 N intervals in ray order: inside [fg_t[i], fg_t[i+1]] (fg_t[N] := far) with mass fg_w[i]; outside, in
    inverse radius, [bg_s[j], bg_s[j+1]] (bg_s[N] := 0: out to infinite radius) with mass bg_lambda bg_w[j], its edges at the
    distance tau(s) = d1 + sqrt(max(1 / s^2 - rho2, 0)) / |d|, d1 = -(o.d) / |d|^2, rho2 = |o + d1 d|^2.  fp64 between fp32 ends.

    Returns dict(opacity (R,) = total mass, disparity (R,) = sum m (1 / a + 1 / b) / 2 over the interval ends as distances
    (1 / inf = 0), distance_percentiles (R, len(quantiles))): +inf where the quantile is not below the opacity (the ray leaves),
    otherwise linear inside its interval - in distance inside the sphere, in inverse radius outside.  quantiles: at most 8,
    ascending, in [0, 1]; a sequence (its device table is kept) or an fp32 device tensor.
    Raises ValueError for shapes, dtypes or devices that do not fit, more than 8 quantiles, or only some of bg_s / bg_w / bg_lambda."""
    if not isinstance(fg_t, torch.Tensor) or fg_t.dim() != 2 or not fg_t.is_cuda:
        raise ValueError("fg_t must be a (R, N) device tensor")
    R, N = fg_t.shape
    dev = fg_t.device
    outside = (bg_s, bg_w, bg_lambda)
    if any(t is None for t in outside) and not all(t is None for t in outside):
        raise ValueError("bg_s, bg_w and bg_lambda go together: give all three, or none for the inside-only histogram")
    if not 1 <= N <= 1024:
        raise ValueError("1 <= N <= 1024 samples per region, got %d" % N)
    fg_t = _extras_row(fg_t, "fg_t", ((R, N),), dev)
    fg_w = _extras_row(fg_w, "fg_w", ((R, N),), dev)
    far = _extras_row(far, "far", ((R,), (R, 1)), dev)
    rays_o = _extras_row(rays_o, "rays_o", ((R, 3),), dev)
    rays_d = _extras_row(rays_d, "rays_d", ((R, 3),), dev)
    if bg_s is not None:
        bg_s = _extras_row(bg_s, "bg_s", ((R, N),), dev)
        bg_w = _extras_row(bg_w, "bg_w", ((R, N),), dev)
        bg_lambda = _extras_row(bg_lambda, "bg_lambda", ((R,), (R, 1)), dev)
    if isinstance(quantiles, torch.Tensor) and (quantiles.device != dev or not quantiles.is_floating_point()):
        raise ValueError("a quantile tensor must be a floating-point tensor on the device of fg_t")
    n_u = quantiles.numel() if isinstance(quantiles, torch.Tensor) else len(quantiles)
    if n_u > MAX_EXTRA_QUANTILES:
        raise ValueError("at most %d quantiles per call, got %d" % (MAX_EXTRA_QUANTILES, n_u))
    tab = _quantile_table(quantiles, dev) if n_u else None
    ctx = _ctx(fg_t, ctx)
    opacity, disparity, pct = torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(R, n_u, device=dev)
    _lib.check(ctx.lib.neo_tp_extras(ctx.handle, ptr(fg_t), ptr(fg_w), ptr(far), ptr(bg_s), ptr(bg_w), ptr(bg_lambda), ptr(rays_o),
                                     ptr(rays_d), R, N, ptr(tab), n_u, ptr(opacity), ptr(disparity), ptr(pct), ctx.stream()))
    return dict(opacity=opacity, disparity=disparity, distance_percentiles=pct)


MAX_EDIT_INSTANCES = 32


def _edit_bounds(near_inst, far_inst, B, dev, who):
    """Validates near_inst / far_inst - (K,B) or (K,B,1) floating-point tensors on `dev`, K <= 32 - and returns K; nothing is
    converted yet (_edit_rows), so that every host-side ValueError comes before the first device access.  `who` names the caller
    in front of every message; None is NeRF_TP.render_instances, whose messages carry no name."""
    pre, like = ("%s: " % who, "") if who else ("", ", like the rays")
    rows = []
    for key, t in (("near_inst", near_inst), ("far_inst", far_inst)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError("%s%s must be a floating-point tensor, got %r" % (pre, key, t.dtype if isinstance(t, torch.Tensor) else type(t).__name__))
        if not (t.dim() in (2, 3) and t.shape[1] == B and (t.dim() == 2 or t.shape[2] == 1)):
            raise ValueError("%s%s must have shape (K, %d) or (K, %d, 1): one row per instance%s, got %s" % (pre, key, B, B, like, tuple(t.shape)))
        if t.shape[0] > MAX_EDIT_INSTANCES:
            raise ValueError("%s%s holds %d instances, at most %d are supported" % (pre, key, t.shape[0], MAX_EDIT_INSTANCES))
        if t.device != dev:
            raise ValueError("%s%s must be on the rays' device (%s), got %s" % (pre, key, dev, t.device))
        rows.append(t)
    if rows[0].shape[0] != rows[1].shape[0]:
        raise ValueError("%snear_inst holds %d instances, far_inst %d" % (pre, rows[0].shape[0], rows[1].shape[0]))
    return rows[0].shape[0]


def _edit_rows(near_inst, far_inst, K, B):
    return f32(near_inst, "near_inst").reshape(K, B), f32(far_inst, "far_inst").reshape(K, B)


def edit_table(K, density_scale=None, tint=None):
    """Host side of an edit: K density scales and K x 3 tints (sequences or CPU tensors; None = all ones) -> two ctypes float arrays
    (or None), validated here - right length, finite, >= 0, else ValueError - and never read from a device."""
    import math
    out = []
    for name, v, width in (("density_scale", density_scale, 1), ("tint", tint, 3)):
        if v is None:
            out.append(None)
            continue
        if isinstance(v, torch.Tensor):
            if v.device.type != "cpu":
                raise ValueError("%s must be a host sequence or a CPU tensor (it travels as a kernel argument), got a tensor on %s" % (name, v.device))
            v = v.detach().tolist()
        rows = [list(r) if width == 3 else [r] for r in v]
        if len(rows) != K or any(len(r) != width for r in rows):
            raise ValueError("%s must hold %s, got %d rows" % (name, "%d values" % K if width == 1 else "%d x 3 values" % K, len(rows)))
        flat = [float(x) for r in rows for x in r]
        if any(not math.isfinite(x) or x < 0.0 for x in flat):
            raise ValueError("%s must be finite and >= 0, got %r" % (name, v))
        out.append((ctypes.c_float * max(len(flat), 1))(*flat))
    return out[0], out[1]


def _floating(who, *named):
    """ValueError for an integer or bool tensor where samples are meant (the conversion to fp32 would hide the mix-up)."""
    for name, v in named:
        if not v.is_floating_point():
            raise ValueError("%s: %s must be a floating-point tensor, got %r" % (who, name, v.dtype))


@torch.no_grad()
def edit_rgbsigma(rgbsigma, t, near_inst, far_inst, density_scale=None, tint=None, ctx=None):
    """The edit of `NeRF_TP.render_edited` on caller rows (neo_tp_edit_rows): an edited COPY of rgbsigma (R,N,4) at the sample rows
    t (R,N).  near_inst / far_inst (K,R) or (K,R,1), K <= 32, ray parameters as `render_objects` reads them; pair (i, ray) is a hit
    by its rule (lo = max(near, 1e-4), hi = far, both finite, hi > lo; a NaN bound is a miss) and sample j is inside iff
    lo <= t_j <= hi.  For i ascending, if inside: sigma *= density_scale[i], rgb *= tint[i] (fp32; overlapping intervals multiply).
    density_scale (K) / tint (K,3): host sequences or CPU tensors, finite and >= 0 (ValueError otherwise), None = ones."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError("t must be a (R, N) tensor")
    R, N = t.shape
    if not isinstance(rgbsigma, torch.Tensor) or tuple(rgbsigma.shape) != (R, N, 4) or rgbsigma.device != t.device:
        raise ValueError("rgbsigma must be a (%d, %d, 4) tensor on the device of t" % (R, N))
    _floating("edit_rgbsigma", ("t", t), ("rgbsigma", rgbsigma))
    K = _edit_bounds(near_inst, far_inst, R, t.device, "edit_rgbsigma")
    scale, tints = edit_table(K, density_scale, tint)
    near_c, far_c = _edit_rows(near_inst, far_inst, K, R)
    out = f32(rgbsigma, "rgbsigma").clone()
    t = f32(t, "t")
    ctx = _ctx(t, ctx)
    if N:
        _lib.check(ctx.lib.neo_tp_edit_rows(ctx.handle, ptr(out), ptr(t), ptr(near_c), ptr(far_c), K, scale, tints, R, N, ctx.stream()))
    return out


def _decomposed_out(K, R, dev):
    """The output tensors of one decomposition and the struct the library writes them through."""
    t = dict(rgb=torch.empty(K + 1, R, 3, device=dev), acc=torch.empty(K + 1, R, device=dev), depth=torch.empty(K + 1, R, device=dev),
             id=torch.empty(R, dtype=torch.int32, device=dev))
    return t, _lib.TpDecomposedOut(*(t[k].data_ptr() for k in ("rgb", "acc", "depth", "id")))


@torch.no_grad()
def decompose_rows(rgbsigma, t, weights, near_inst, far_inst, bg_lambda=None, ctx=None):
    """The decomposition of `NeRF_TP.render_decomposed` on caller rows (neo_tp_decompose_rows; the DECOMPOSITION RULE of
    include/neo360_hip.h): rgbsigma (R,N,4), the sample rows t (R,N), and the scene weights (R,N) as `composite(1, ...)` returns
    them; near_inst / far_inst (K,R) or (K,R,1), K <= 32, ray parameters as `render_objects` reads them; bg_lambda None, (R,) or
    (R,1).  Pair (i, ray) is a hit by the rule of `render_objects` (lo = max(near, 1e-4), hi = far, both finite, hi > lo; a NaN
    bound is a miss); sample j is inside iff lo <= t_j <= hi, and belongs to the lowest-indexed hit pair it is inside of, else to
    slot K, the rest.  Returns dict(rgb (K+1,R,3), acc (K+1,R), depth (K+1,R), id (R,) int32): per slot the sums of w c, w and w t
    over its samples in `composite`'s own fp32 order (a slot that owns a whole ray is bitwise `composite(1, ...)`, one that owns
    nothing is exactly 0), and id = the instance with the largest acc (ties: lower index) iff that is > 0 and >= acc[K] + bg_lambda,
    else -1.  1 <= N <= 1024.  Raises ValueError for shapes, dtypes or devices that do not fit and for K > 32."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or not t.is_floating_point() or not t.is_cuda:
        raise ValueError("t must be a floating-point (R, N) device tensor")
    R, N = t.shape
    dev = t.device
    if not 1 <= N <= 1024:
        raise ValueError("1 <= N <= 1024 samples per ray, got %d" % N)
    for name, v, want in (("rgbsigma", rgbsigma, ((R, N, 4),)), ("weights", weights, ((R, N),)), ("bg_lambda", bg_lambda, ((R,), (R, 1)))):
        if v is None and name == "bg_lambda":
            continue
        if not isinstance(v, torch.Tensor) or not v.is_floating_point():
            raise ValueError("%s must be a floating-point tensor, got %r" % (name, v.dtype if isinstance(v, torch.Tensor) else type(v).__name__))
        if tuple(v.shape) not in want:
            raise ValueError("%s must have shape %s, got %s" % (name, " or ".join(str(s) for s in want), tuple(v.shape)))
        if v.device != dev:
            raise ValueError("%s must be on the device of t (%s), got %s" % (name, dev, v.device))
    K = _edit_bounds(near_inst, far_inst, R, dev, "decompose_rows")
    near_c, far_c = _edit_rows(near_inst, far_inst, K, R)
    rgbsigma, t, weights = f32(rgbsigma, "rgbsigma"), f32(t, "t"), f32(weights, "weights")
    lam = f32(bg_lambda, "bg_lambda").reshape(R) if bg_lambda is not None else None
    ctx = _ctx(t, ctx)
    out, struct = _decomposed_out(K, R, dev)
    _lib.check(ctx.lib.neo_tp_decompose_rows(ctx.handle, ptr(rgbsigma), ptr(t), ptr(weights), ptr(near_c), ptr(far_c), K, R, N, ptr(lam),
                                             ctypes.byref(struct), ctx.stream()))
    return out


def _layer_rows(layers, B, dev, who):
    """Validates layers = None or dict(key (L,B), rgb (L,B,3), acc (L,B), depth (L,B)) on `dev`, L <= 32, and returns L; nothing is
    converted yet (_layer_struct)."""
    if layers is None:
        return 0
    if not hasattr(layers, "keys") or any(k not in layers for k in ("key", "rgb", "acc", "depth")):
        raise ValueError("%s: layers must be a dict with key (L,B), rgb (L,B,3), acc (L,B) and depth (L,B)" % who)
    L = layers["key"].shape[0] if isinstance(layers["key"], torch.Tensor) and layers["key"].dim() == 2 else -1
    for k in ("key", "rgb", "acc", "depth"):
        v = layers[k]
        want = (L, B, 3) if k == "rgb" else (L, B)
        if not isinstance(v, torch.Tensor) or not v.is_floating_point():
            raise ValueError("%s: layers[%r] must be a floating-point tensor" % (who, k))
        if L < 0 or tuple(v.shape) != want:
            raise ValueError("%s: layers[%r] must have shape %s, got %s" % (who, k, "(L, %d%s)" % (B, ", 3" if k == "rgb" else ""), tuple(v.shape)))
        if v.device != dev:
            raise ValueError("%s: layers[%r] must be on the rays' device (%s), got %s" % (who, k, dev, v.device))
    if L > MAX_EDIT_INSTANCES:
        raise ValueError("%s: %d layers, at most %d are supported" % (who, L, MAX_EDIT_INSTANCES))
    return L


def _layer_struct(layers, L):
    """The fp32 rows of validated layers and the struct the library reads them through: ((), None) when L == 0."""
    if not L:
        return (), None
    rows = tuple(f32(layers[k], k) for k in ("key", "rgb", "acc", "depth"))
    return rows, _lib.TpLayers(*(r.data_ptr() for r in rows))


@torch.no_grad()
def composite_layers(rgbsigma, t, rays_d, t_far, layers, ctx=None):
    """`composite(1, ...)` with up to 32 per-ray layers spliced into the ray (neo_composite_layers; the LAYER RECURRENCE of
    include/neo360_hip.h).  t (R,N) defines R and N; rgbsigma (R,N,4), rays_d (R,3), t_far (R,) or (R,1): any float dtype, any
    strides.  layers: dict(key (L,R) ray parameters, rgb (L,R,3) premultiplied colours, acc (L,R) opacities, depth
    (L,R) premultiplied depths) or None.  A layer is valid iff its key is finite and its acc > 0; valid layers act in ascending key
    (ties: lower index) as slabs with keep = max(1 - acc, 0) placed before the first sample at or beyond their key.
    Returns dict(rgb, acc, depth, weights, bg_lambda, visibility (L,R)); `weights` are the scene's own (those of `composite`), and
    with no valid layer everything is bitwise `composite(1, ...)`."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError("t must be a (R, N) tensor")
    R, N = t.shape
    dev = t.device
    L = _layer_rows(layers, R, dev, "composite_layers")
    rgbsigma, t, rays_d, t_far = _composite_args(1, rgbsigma, t, rays_d, t_far)
    if rays_d is None or t_far is None:
        raise ValueError("composite_layers: rays_d must have shape (%d, 3) and t_far (%d,) or (%d, 1), got None" % (R, R, R))
    ctx = _ctx(t, ctx)
    rows, struct = _layer_struct(layers, L)
    rgb = torch.empty(R, 3, device=dev)
    acc = torch.empty(R, device=dev)
    depth = torch.empty(R, device=dev)
    w = torch.empty(R, N, device=dev)
    lam = torch.empty(R, 1, device=dev)
    vis = torch.empty(L, R, device=dev)
    _lib.check(ctx.lib.neo_composite_layers(ctx.handle, ptr(rgbsigma), ptr(t), ptr(rays_d), ptr(t_far), R, N,
                                            ctypes.byref(struct) if struct is not None else None, L, ptr(rgb), ptr(acc), ptr(depth),
                                            ptr(w), ptr(lam), ptr(vis) if L else None, ctx.stream()))
    return dict(rgb=rgb, acc=acc, depth=depth, weights=w, bg_lambda=lam, visibility=vis)


def occupancy_resolution_ok(G):
    """The resolutions an occupancy grid may have: 8 and 16 (tests), or a multiple of 32 in [32, 256]."""
    return isinstance(G, int) and not isinstance(G, bool) and (G in (8, 16) or (32 <= G <= 256 and G % 32 == 0))


def _check_occupancy(occ, who):
    """ValueError unless occ is a bool (G,G,G) tensor of a supported G; returns G.  Touches no device."""
    if not isinstance(occ, torch.Tensor) or occ.dtype != torch.bool:
        raise ValueError("%s: the occupancy grid must be a bool tensor, got %r" % (who, occ.dtype if isinstance(occ, torch.Tensor) else type(occ).__name__))
    if occ.dim() != 3 or not (occ.shape[0] == occ.shape[1] == occ.shape[2]):
        raise ValueError("%s: the occupancy grid must have shape (G, G, G), got %s" % (who, tuple(occ.shape)))
    G = int(occ.shape[0])
    if not occupancy_resolution_ok(G):
        raise ValueError("%s: G must be 8, 16 or a multiple of 32 in [32, 256], got %d" % (who, G))
    return G


def pack_occupancy(occ):
    """bool (G,G,G) -> int32 (G^3 / 32,) on the same device, the layout the library reads (include/neo360_hip.h, OCCUPANCY GRID):
    cell (ix, iy, iz) is bit lin & 31 of word lin >> 5, lin = (ix G + iy) G + iz."""
    _check_occupancy(occ, "pack_occupancy")
    b = occ.contiguous().reshape(-1, 32).to(torch.int64)
    words = (b << torch.arange(32, dtype=torch.int64, device=occ.device)).sum(dim=-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)           # the same 32 bits as a signed word
    return words.to(torch.int32)


def unpack_occupancy(words, G):
    """The inverse of pack_occupancy: int32 (G^3 / 32,) -> bool (G,G,G)."""
    if not occupancy_resolution_ok(G):
        raise ValueError("unpack_occupancy: G must be 8, 16 or a multiple of 32 in [32, 256], got %r" % (G,))
    if not isinstance(words, torch.Tensor) or words.dtype != torch.int32 or words.numel() != G ** 3 // 32:
        raise ValueError("unpack_occupancy: expected %d int32 words" % (G ** 3 // 32))
    w = words.reshape(-1, 1).to(torch.int64)
    return ((w >> torch.arange(32, dtype=torch.int64, device=words.device)) & 1).to(torch.bool).reshape(G, G, G)


@torch.no_grad()
def occupancy_keep(occ, rays_o, rays_d, t, ctx=None):
    """The KEEP RULE of `NeRF_TP.render_skipping` on caller rows (neo_tp_occupancy_keep): occ bool (G,G,G) on any device, or None
    for "no grid"; rays_o, rays_d (B,3) and t (B,N) on the GPU.  Sample j of ray b, at x = rays_o[b] + t[b, j] * rays_d[b] in fp32,
    is kept iff the cell of x - per axis min(max(floor((x + 1) * (G / 2)), 0), G - 1), in fp32 - is set, or a coordinate of x is
    not finite, or occ is None.  Returns (B,N) bool."""
    if occ is not None:
        _check_occupancy(occ, "occupancy_keep")
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or not t.is_floating_point():
        raise ValueError("occupancy_keep: t must be a floating-point (B, N) tensor")
    B, N = t.shape
    for name, v in (("rays_o", rays_o), ("rays_d", rays_d)):
        if not isinstance(v, torch.Tensor) or tuple(v.shape) != (B, 3) or v.device != t.device:
            raise ValueError("occupancy_keep: %s must be a (%d, 3) tensor on the device of t" % (name, B))
    if N < 1:
        raise ValueError("occupancy_keep: at least one sample per ray")
    _floating("occupancy_keep", ("rays_o", rays_o), ("rays_d", rays_d))
    rays_o, rays_d, t = f32(rays_o, "rays_o"), f32(rays_d, "rays_d"), f32(t, "t")
    ctx = _ctx(t, ctx)
    bits = pack_occupancy(occ.to(t.device)) if occ is not None else None
    keep = torch.empty(B, N, dtype=torch.bool, device=t.device)
    _lib.check(ctx.lib.neo_tp_occupancy_keep(ctx.handle, ptr(bits), int(occ.shape[0]) if occ is not None else 0, ptr(rays_o),
                                             ptr(rays_d), ptr(t), B, N, keep.data_ptr(), ctx.stream()))
    return keep


def occupancy_lattice(resolution, probes, device="cpu"):
    """The probe positions of `NeRF_TP.build_occupancy`: the M = resolution * probes sub-centres -1 + (l + 1/2) * 2 / M of one axis
    (fp64, rounded to fp32), and the lattice as rays - column (lx, ly) is the ray o = (c[lx], c[ly], 0), d = (0, 0, 1) sampled at
    t = c, so that o + t d is the lattice point exactly.  Returns (c (M,), rays_o (M^2,3), rays_d (M^2,3))."""
    M = int(resolution) * int(probes)
    c = (-1.0 + (torch.arange(M, dtype=torch.float64) + 0.5) * (2.0 / M)).float().to(device)
    rays_o = torch.stack([c[:, None].expand(M, M), c[None, :].expand(M, M), torch.zeros(M, M, device=device)], dim=-1).reshape(M * M, 3)
    rays_d = torch.tensor([0.0, 0.0, 1.0], device=device).expand(M * M, 3).contiguous()
    return c, rays_o.contiguous(), rays_d


@torch.no_grad()
def occupancy_from_sigma(sigma, resolution, sigma_threshold, probes=2, dilate=1, ctx=None):
    """A lattice of activated densities -> a bool (G,G,G) grid (neo_occupancy_from_sigma).  sigma: (M,M,M) on the GPU, M =
    resolution * probes, entry (lx, ly, lz) a probe of cell (lx // probes, ly // probes, lz // probes).  A cell is occupied iff a
    probe of a cell within `dilate` cells of it in every axis is not <= sigma_threshold (a NaN density is occupied), and cleared
    when no point of it lies inside the unit sphere."""
    G, probes, dilate = _check_build(resolution, sigma_threshold, probes, dilate, "occupancy_from_sigma")
    M = G * probes
    if not isinstance(sigma, torch.Tensor) or tuple(sigma.shape) != (M, M, M) or not sigma.is_floating_point():
        raise ValueError("occupancy_from_sigma: sigma must be a floating-point (%d, %d, %d) tensor" % (M, M, M))
    sigma = f32(sigma, "sigma")
    ctx = _ctx(sigma, ctx)
    bits = torch.empty(G ** 3 // 32, dtype=torch.int32, device=sigma.device)
    _lib.check(ctx.lib.neo_occupancy_from_sigma(ctx.handle, ptr(sigma), G, probes, float(sigma_threshold), dilate, ptr(bits), ctx.stream()))
    return unpack_occupancy(bits, G)


def _check_build(resolution, sigma_threshold, probes, dilate, who):
    import math
    if not occupancy_resolution_ok(resolution):
        raise ValueError("%s: resolution must be 8, 16 or a multiple of 32 in [32, 256], got %r" % (who, resolution))
    for name, v, lo, hi in (("probes", probes, 1, 4), ("dilate", dilate, 0, 4)):
        if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
            raise ValueError("%s: %s must be an integer in [%d, %d], got %r" % (who, name, lo, hi, v))
    if isinstance(sigma_threshold, bool) or not isinstance(sigma_threshold, (int, float)) or math.isnan(float(sigma_threshold)):
        raise ValueError("%s: sigma_threshold must be a number, got %r" % (who, sigma_threshold))
    return int(resolution), int(probes), int(dilate)


def _check_termination(eps, segment, who):
    """eps in [0, 1) (NaN refused), segment a positive multiple of 64: ValueError before any device access."""
    import math
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or math.isnan(float(eps)) or not 0.0 <= float(eps) < 1.0:
        raise ValueError("%s: eps must be a number in [0, 1), got %r" % (who, eps))
    if isinstance(segment, bool) or not isinstance(segment, int) or segment < 64 or segment % 64 != 0:
        raise ValueError("%s: segment must be a positive multiple of 64, got %r" % (who, segment))
    return float(eps), int(segment)


@torch.no_grad()
def termination_stops(rgbsigma, t, rays_d, t_far, eps, segment=64, ctx=None):
    """The STOP RULE of `NeRF_TP.render_terminating` on caller rows (neo_tp_termination_stops): rgbsigma (B,N,4), t (B,N), rays_d
    (B,3), t_far (B,) or (B,1) on the GPU - what `eval_mlp` returns for the inside-sphere samples of a level and what the
    inside-sphere `composite` reads.  The N samples are cut into segments of `segment` (a positive multiple of 64); a march evaluates
    segment 0, and segment k >= 1 iff at every earlier boundary b the transmittance in front of sample b - the composite's own
    (float)carry, formed with its expressions - was not below eps (a NaN keeps marching).  Returns (stop (B,) int32, the number of
    leading samples such a march evaluates, and trans (B,) float32, the transmittance at the stop).  stop.sum() / (B N) is the share
    of a level's inside-sphere work the rule would keep: the tool to measure it on trained weights without the frame call."""
    eps, segment = _check_termination(eps, segment, "termination_stops")
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or not t.is_floating_point() or t.shape[1] < 1:
        raise ValueError("termination_stops: t must be a floating-point (B, N) tensor, N >= 1")
    B, N = t.shape
    if not isinstance(rgbsigma, torch.Tensor) or tuple(rgbsigma.shape) != (B, N, 4) or rgbsigma.device != t.device:
        raise ValueError("termination_stops: rgbsigma must be a (%d, %d, 4) tensor on the device of t" % (B, N))
    if not isinstance(rays_d, torch.Tensor) or tuple(rays_d.shape) != (B, 3) or rays_d.device != t.device:
        raise ValueError("termination_stops: rays_d must be a (%d, 3) tensor on the device of t" % B)
    if not isinstance(t_far, torch.Tensor) or tuple(t_far.shape) not in ((B,), (B, 1)) or t_far.device != t.device:
        raise ValueError("termination_stops: t_far must be a (%d,) or (%d, 1) tensor on the device of t" % (B, B))
    _floating("termination_stops", ("rgbsigma", rgbsigma), ("rays_d", rays_d), ("t_far", t_far))
    rgbsigma, t, rays_d, t_far = f32(rgbsigma, "rgbsigma"), f32(t, "t"), f32(rays_d, "rays_d"), f32(t_far.reshape(B), "t_far")
    ctx = _ctx(t, ctx)
    stop = torch.empty(B, dtype=torch.int32, device=t.device)
    trans = torch.empty(B, device=t.device)
    _lib.check(ctx.lib.neo_tp_termination_stops(ctx.handle, ptr(rgbsigma), ptr(t), ptr(rays_d), ptr(t_far), B, N, eps, segment,
                                                stop.data_ptr(), trans.data_ptr(), ctx.stream()))
    return stop, trans


@torch.no_grad()
def termination_stops_outside(rgbsigma, s, bg_lambda, eps, segment=64, ctx=None):
    """The OUTSIDE STOP RULE of `NeRF_TP.render_marching` on caller rows (neo_tp_termination_stops_outside): rgbsigma (B,N,4) and
    s (B,N) on the GPU - what `eval_mlp` returns for the outside-sphere samples of a level and the descending 1/r positions the
    outside-sphere `composite` (mode 2) reads - and bg_lambda (B,) or (B,1), the level's foreground leftover.  The N samples are cut
    into segments of `segment` (a positive multiple of 64); a march evaluates segment 0, and segment k >= 1 iff at every earlier
    boundary b the running value v_b = bg_lambda * (float)carry_b - one fp32 multiply with the composite's own background
    transmittance in front of sample b - was not below eps (a NaN keeps marching).  Every row counts as a ray whose background runs.
    Returns (stop (B,) int32, the leading samples such a march evaluates, and value (B,) float32, v at the stop).
    stop.sum() / (B N) is the share of a level's outside-sphere work the rule would keep: the tool to measure it on trained weights
    without the frame call."""
    eps, segment = _check_termination(eps, segment, "termination_stops_outside")
    if not isinstance(s, torch.Tensor) or s.dim() != 2 or not s.is_floating_point() or s.shape[1] < 1:
        raise ValueError("termination_stops_outside: s must be a floating-point (B, N) tensor, N >= 1")
    B, N = s.shape
    if not isinstance(rgbsigma, torch.Tensor) or tuple(rgbsigma.shape) != (B, N, 4) or rgbsigma.device != s.device:
        raise ValueError("termination_stops_outside: rgbsigma must be a (%d, %d, 4) tensor on the device of s" % (B, N))
    if not isinstance(bg_lambda, torch.Tensor) or tuple(bg_lambda.shape) not in ((B,), (B, 1)) or bg_lambda.device != s.device:
        raise ValueError("termination_stops_outside: bg_lambda must be a (%d,) or (%d, 1) tensor on the device of s" % (B, B))
    _floating("termination_stops_outside", ("rgbsigma", rgbsigma), ("bg_lambda", bg_lambda))
    rgbsigma, s, bg_lambda = f32(rgbsigma, "rgbsigma"), f32(s, "s"), f32(bg_lambda.reshape(B), "bg_lambda")
    ctx = _ctx(s, ctx)
    stop = torch.empty(B, dtype=torch.int32, device=s.device)
    value = torch.empty(B, device=s.device)
    _lib.check(ctx.lib.neo_tp_termination_stops_outside(ctx.handle, ptr(rgbsigma), ptr(s), ptr(bg_lambda), B, N, eps, segment,
                                                        stop.data_ptr(), value.data_ptr(), ctx.stream()))
    return stop, value
