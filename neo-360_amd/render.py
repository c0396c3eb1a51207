"""Whole-frame rendering: the counterpart of the reference's Lit*.render_rays_test
chunk loops (vanilla_nerf/model.py:336-363, neo360/model.py:861-907) without the
Python loop — one library call per frame (or per rank's shard of it), with the
reference chunk size passed down so NeO-360's chunk-dependent view-direction tiling
is reproduced — plus the single-frame replacement of the reference's only collective
(LitModel.alter_gather_cat, models/interface.py:30-50) and its PSNR (:53-61).
"""
import math
import warnings

import torch

from . import _lib, models
from .context import dense, radii_shapes, ray_rows
from .parallel import gather_tiles, shard_bounds

_WHOLE = ("src_imgs", "src_poses", "src_focal", "src_c")


def _slice(batch, lo, hi):
    out = {}
    for k, v in batch.items():
        if k in _WHOLE or not isinstance(v, torch.Tensor):
            out[k] = v
        elif k == "radii" and v.dim() == 2 and v.shape[0] == 1:
            out[k] = v[:, lo:hi]
        else:
            out[k] = v[lo:hi]
    return out


def _render_once(model, batch, chunk, white_bkgd, near, far, train_frac):
    if isinstance(model, models.NeRF_TP):
        res = model(batch, False, white_bkgd, near, far, out_depth=True, chunk=chunk, fine_only=True)      # only res[1] is read
        out = dict(rgb=res[1][0], depth=res[1][5], fg_rgb=res[1][1], bg_rgb=res[1][2], acc=res[1][3])
        if model.compute_extras:            # the fine level's extras ride along; every other key keeps its meaning
            extras = res[1][6]
            named = ("distance_median", "distance_percentile_5", "distance_percentile_95")
            for k in ("opacity", "disparity") + (named if named[0] in extras else ("distance_percentiles",)):
                out[k] = extras[k]
        return out
    if isinstance(model, models.PixelNeRF):
        res = model(batch, False, white_bkgd, near, far, chunk=chunk)      # vanilla_nerf/model_pixel.py:356-383
        return dict(rgb=res[1][0], depth=res[1][2], acc=res[1][1])
    if isinstance(model, models.MipNeRF360):
        # mipnerf360/model.py:471-505: train_frac = global_step / max_steps of the trainer; near/far as given
        rend, hist = model(batch, train_frac, False, False, near, far)
        last = rend[-1]
        if model.compute_extras:            # depth = the expected distance of the final level, acc the kernel's own sum
            return dict(rgb=last["rgb"], acc=last["acc"], depth=last["distance_mean"], distance_median=last["distance_median"],
                        distance_percentile_5=last["distance_percentile_5"], distance_percentile_95=last["distance_percentile_95"])
        w = hist[-1]["weights"]
        return dict(rgb=last["rgb"], acc=w.sum(-1), depth=torch.zeros_like(w[:, 0]))   # the reference returns rgb only
    if isinstance(model, models.NeRF):
        res = model(batch, False, white_bkgd, near, far)     # chunking does not change vanilla results
        return dict(rgb=res[1][0], depth=res[1][2], acc=res[1][1])
    raise TypeError("unsupported renderer %r" % type(model))


def _render_exact(model, once):
    prev = model.precision
    model.precision = "f32"
    try:
        out = once()
        model.check_flags()
    finally:
        model.precision = prev
    out["precision_used"] = "f32"
    return out


def _render_guarded(model, batch, once, check, on_range):
    """One frame through `once()` (a callable that renders it once in the module's current arithmetic and returns the output
    dict) with the range-guard retry and latch of render_rays_test / render_object_rays (documented there); `target` /
    `instance_mask` of the batch are passed through."""
    if on_range not in ("retry_f32", "raise"):
        raise ValueError("on_range must be 'retry_f32' or 'raise', got %r" % (on_range,))
    latch = getattr(model, "_range_latch", None)
    if latch is not None and on_range == "retry_f32" and check and (model.precision or model.default_precision) != "f32":
        if latch == model.operands_key():
            out = _render_exact(model, once)
            model.last_precision_used = "f32"
            for k in ("target", "instance_mask"):
                if k in batch:
                    out[k] = batch[k]
            return out
        model._range_latch = None          # weights or scene changed: the split arithmetic gets another chance
    out = once()
    model.last_precision_used = model.precision or model.default_precision
    if check:
        try:
            model.check_flags()      # the deferred reads of the assertion word: raise before the frame is handed out
        except _lib.NeoRangeError as err:
            if on_range != "retry_f32":
                raise
            if not getattr(model, "_warned_range_downgrade", False):
                model._warned_range_downgrade = True
                warnings.warn("%s: an operand left the fp16 range of the split arithmetic (precision 'f16x3'); this frame "
                              "(and any later one that trips the guard) is re-rendered on the exact fp32 kernels "
                              "(~3-6x slower). Set model.precision = 'f32' to skip the failed attempt."
                              % type(model).__name__, RuntimeWarning, stacklevel=3)
            if getattr(err, "static_operand", False):
                model._range_latch = model.operands_key()
            out = _render_exact(model, once)
            model.last_precision_used = "f32"
    for k in ("target", "instance_mask"):
        if k in batch:
            out[k] = batch[k]
    return out


@torch.no_grad()
def render_rays_test(model, batch, chunk=1024, white_bkgd=False, near=0.2, far=3.0, train_frac=1.0, check=True,
                     on_range="retry_f32", image_width=None, first_ray=0):
    """Fine-level rgb / depth of every ray in `batch` (one image), as the reference's
    render_rays_test returns them: dict(rgb (R,3), depth (R,)) plus `target` /
    `instance_mask` passed through when present.  A MipNeRF360 returns depth = 0 (the reference renders rgb only) unless
    `model.compute_extras` is set: then depth = the final level's expected distance (`distance_mean`), acc the kernel's own
    sum, and `distance_median` / `distance_percentile_5` / `distance_percentile_95` ride along.  A NeRF_TP with
    `model.compute_extras` set adds `opacity`, `disparity`, `distance_median`, `distance_percentile_5` and `distance_percentile_95`
    of the fine level (distances along the ray, in the unit of the ray parameter t of o + t d; `distance_percentiles` instead of the
    three named ones when `model.extras_quantiles` is not the default); `depth` and `acc` stay the reference's composite depth and
    the foreground's opacity.  check=True waits for the frame and raises what the device-side
    assertions reported (a ray that missed the unit sphere); check=False leaves that to
    a later `model.check_flags()` (a loop over frames that never wants to block).

    on_range: what happens when the range guard of the split-fp16 arithmetic trips for this frame (an operand beyond the
    fp16 range: a trained checkpoint or an un-normalised encoder; the reference is plain fp32 and never fails,
    neo360/model.py:343-407).  "retry_f32" (default): the frame is rendered again on the exact fp32-MFMA kernels of the
    same library - bitwise the frame `model.precision = "f32"` returns - and a RuntimeWarning says so once per module
    (the flag lives ON the module); "raise": the NeoRangeError goes to the caller.  Needs check=True (the guard is read when
    the frame is complete).  When the operand that left the range is a STATIC one (packed weights, an uploaded feature map:
    `NeoRangeError.static_operand`) every later frame would trip again, so the module is LATCHED: until its parameters or
    its scene change (`model.operands_key()`), frames go straight to the exact kernels - one render per frame, not a failed
    split attempt plus a retry.  A trip on activations is per frame and is not latched.  `out["precision_used"] = "f32"`
    marks such frames; `model.last_precision_used` holds the arithmetic of the last frame either way."""
    if on_range not in ("retry_f32", "raise"):
        raise ValueError("on_range must be 'retry_f32' or 'raise', got %r" % (on_range,))
    if image_width and isinstance(model, models.NeRF_TP):
        # image_width (+ first_ray: the frame index of this batch's first ray, for a rank's shard): the rays are the row-major
        # pixels of an image - the evaluators then walk them in 8 x 8 pixel patches (neo_ctx_set_ray_grid: L2 locality in both
        # image directions, bitwise the same frame)
        prev_grid = getattr(model, "ray_grid", None)
        model.ray_grid = (int(image_width), int(first_ray))
        try:
            return render_rays_test(model, batch, chunk, white_bkgd, near, far, train_frac, check, on_range)
        finally:
            model.ray_grid = prev_grid
    return _render_guarded(model, batch, lambda: _render_once(model, batch, chunk, white_bkgd, near, far, train_frac), check, on_range)


@torch.no_grad()
def render_object_rays(model, batch, chunk=1024, white_bkgd=True, check=True, on_range="retry_f32"):
    """Object-level frame of a NeRF_TP module: the fine level of `model.render_objects` on every ray of `batch` (which carries
    the reference's `near_obj` / `far_obj` keys, e.g. from ops.sample_rays_in_bbox) in one library call, with the reference
    chunk size passed down.  Returns dict(rgb (R,3), depth (R,), acc (R,)) plus `target` / `instance_mask` passed through.
    Rays without a box interval return the background colour (white_bkgd) and acc = depth = 0.  check / on_range: the flag
    read, range-guard retry and latch of render_rays_test (the same code path)."""
    if not isinstance(model, models.NeRF_TP):
        raise TypeError("render_object_rays renders NeRF_TP modules, got %r" % type(model))

    def once():
        res = model.render_objects(batch, white_bkgd=white_bkgd, chunk=chunk)
        return dict(rgb=res[1][0], depth=res[1][2], acc=res[1][1])
    return _render_guarded(model, batch, once, check, on_range)


@torch.no_grad()
def render_instance_rays(model, batch, RTs=None, chunk=1024, white_bkgd=True, check=True, on_range="retry_f32"):
    """Instance-level frame of a NeRF_TP module: the fine level of `model.render_instances` on every ray of `batch` in one
    library call, with the reference chunk size passed down.  The per-instance intervals are batch["near_inst"] /
    batch["far_inst"] ((K,R) or (K,R,1)) when present, else they are computed from `RTs` (the reference's dict of boxes) with
    ops.sample_rays_in_bbox_list.  Returns dict(rgb (R,3), depth (R,), acc (R,), instance_id (R,) int32) - the depth-ordered
    composite of the instances and the visible instance of every ray (-1: none) - plus `instances` = (rgb (K,R,3), acc (K,R),
    depth (K,R)), row i bitwise render_object_rays on instance i's interval, and `target` / `instance_mask` passed through.
    check / on_range: the flag read, range-guard retry and latch of render_rays_test (the same code path)."""
    if not isinstance(model, models.NeRF_TP):
        raise TypeError("render_instance_rays renders NeRF_TP modules, got %r" % type(model))
    if "near_inst" in batch and "far_inst" in batch:
        near, far = batch["near_inst"], batch["far_inst"]
    elif RTs is not None:
        from . import ops
        near, far, _ = ops.sample_rays_in_bbox_list(RTs, batch["rays_o"], batch["viewdirs"])
    else:
        raise ValueError("render_instance_rays needs the per-instance intervals: batch['near_inst'] / batch['far_inst'], or RTs")

    def once():
        res = model.render_instances(batch, near, far, white_bkgd=white_bkgd, chunk=chunk)
        rgb, acc, depth, ids = res["composite"][1]
        return dict(rgb=rgb, depth=depth, acc=acc, instance_id=ids, instances=res["instances"][1])
    return _render_guarded(model, batch, once, check, on_range)


def _rigid(M, index):
    """A 4x4 rigid world transform as fp64 (rotation, translation); ValueError when it is not one."""
    m = torch.as_tensor(M, dtype=torch.float64, device="cpu")
    if tuple(m.shape) != (4, 4) or not bool(torch.isfinite(m).all()):
        raise ValueError("moves[%r] must be a finite 4x4 matrix" % (index,))
    rot, tran = m[:3, :3], m[:3, 3]
    rigid = (float((rot @ rot.T - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6 and abs(float(torch.linalg.det(rot)) - 1.0) <= 1e-6
             and float((m[3] - torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)).abs().max()) <= 1e-12)
    if not rigid:
        raise ValueError("moves[%r] is not a rigid transform (orthonormal rotation with det +1, last row 0 0 0 1)" % (index,))
    return rot, tran


def _check_moves(moves, K):
    out = {}
    for i, M in (moves or {}).items():
        if not isinstance(i, int) or isinstance(i, bool) or not 0 <= i < K:
            raise ValueError("moves: %r is not an instance index in [0, %d)" % (i, K))
        out[i] = _rigid(M, i)
    return dict(sorted(out.items()))


@torch.no_grad()
def instance_layers(model, batch, RTs, moves, chunk=1024):
    """Instances of a NeRF_TP scene rendered SOMEWHERE ELSE, as the layers `NeRF_TP.render_edited` takes.  moves: {instance index
    into RTs: 4x4 rigid world transform M, new = M * old} (ValueError for a non-rigid M).  Seeing the moved instance along a ray is
    seeing the instance where it stands along the ray moved back: per moved instance o' = Rm^T (o - tm), d' = Rm^T d, viewdirs' =
    Rm^T viewdirs, in fp64 and rounded to fp32; its box interval from `ops.sample_rays_in_bbox_list` on those rays (|Rm^T d| = |d|:
    the ray parameter is unchanged); the fine level of `render_objects(..., white_bkgd=False)` on them is the layer, key = lo where
    the pair is hit, else +inf.  The moved instance keeps the lighting and the quirk-Q1 direction row of its transformed ray.
    Returns dict(key (L,R), rgb (L,R,3), acc (L,R), depth (L,R), index = the moved instance indices, ascending)."""
    if not isinstance(model, models.NeRF_TP):
        raise TypeError("instance_layers renders NeRF_TP modules, got %r" % type(model))
    from . import ops
    K = len(RTs["R"])
    moves = _check_moves(moves, K)
    ray_rows(batch)         # rays_o defines R: the moved rays below are formed per tensor, so a tensor of another frame is refused first
    dev = batch["rays_o"].device
    R = batch["rays_o"].shape[0]
    out = dict(key=[], rgb=[], acc=[], depth=[])
    for i, (rot, tran) in moves.items():
        rot_d, tran_d = rot.to(dev), tran.to(dev)
        moved = dict(batch)
        moved["rays_o"] = ((batch["rays_o"].double() - tran_d) @ rot_d).float()        # row vectors: x Rm = (Rm^T x^T)^T
        moved["rays_d"] = (batch["rays_d"].double() @ rot_d).float()
        moved["viewdirs"] = (batch["viewdirs"].double() @ rot_d).float()
        one = dict(R=[RTs["R"][i]], T=[RTs["T"][i]], s=[RTs["s"][i]])
        near, far, _ = ops.sample_rays_in_bbox_list(one, moved["rays_o"], moved["viewdirs"])
        near, far = near.reshape(R), far.reshape(R)
        rgb, acc, depth = model.render_objects(moved, near_obj=near, far_obj=far, white_bkgd=False, chunk=chunk)[1]
        lo = torch.clamp(near, min=1e-4)
        hit = torch.isfinite(near) & torch.isfinite(far) & (far > lo)
        out["key"].append(torch.where(hit, lo, torch.full_like(lo, float("inf"))))
        out["rgb"].append(rgb)
        out["acc"].append(acc)
        out["depth"].append(depth)
    layers = {k: (torch.stack(v) if v else torch.empty((0, R, 3) if k == "rgb" else (0, R), device=dev)) for k, v in out.items()}
    layers["index"] = list(moves)
    return layers


@torch.no_grad()
def render_edited_rays(model, batch, RTs=None, density_scale=None, tint=None, moves=None, chunk=1024, check=True,
                       on_range="retry_f32"):
    """Edited frame of a NeRF_TP module: the fine level of `model.render_edited` on every ray of `batch` in one library call, with
    the reference chunk size passed down.  The per-instance intervals are batch["near_inst"] / batch["far_inst"] when present, else
    they are computed from `RTs` with ops.sample_rays_in_bbox_list.  density_scale (K) / tint (K x 3): host sequences, as
    `render_edited` takes them.  moves ({instance index: 4x4 rigid M}, needs RTs): those instances are rendered where M puts them,
    as layers (`instance_layers`), and get density scale 0 in the scene pass; a scale or tint other than 1 given for a moved
    instance raises ValueError.  Everything runs inside one guarded render (check / on_range: the flag read, range-guard retry and
    latch of render_rays_test).  Returns dict(rgb (R,3), depth (R,), acc (R,), bg_lambda (R,1)[, visibility (L,R)]) of the fine
    level plus `target` / `instance_mask` passed through; with the defaults rgb / depth are bitwise render_rays_test's."""
    if not isinstance(model, models.NeRF_TP):
        raise TypeError("render_edited_rays renders NeRF_TP modules, got %r" % type(model))
    if on_range not in ("retry_f32", "raise"):
        raise ValueError("on_range must be 'retry_f32' or 'raise', got %r" % (on_range,))
    from . import ops
    if moves and RTs is None:
        raise ValueError("render_edited_rays needs RTs to render moved instances")
    given = "near_inst" in batch and "far_inst" in batch
    K = batch["near_inst"].shape[0] if given else len(RTs["R"]) if RTs is not None else 0
    if given and RTs is not None and len(RTs["R"]) != K:
        raise ValueError("RTs holds %d boxes, the batch's intervals %d instances" % (len(RTs["R"]), K))
    moved = _check_moves(moves, K)
    scale, tints = ops.edit_table(K, density_scale, tint)      # validation only: render_edited builds its own tables
    scale = [1.0] * K if scale is None else list(scale)[:K]
    tints = [[1.0, 1.0, 1.0] for _ in range(K)] if tints is None else [list(tints)[3 * i:3 * i + 3] for i in range(K)]
    for i in moved:
        if scale[i] != 1.0 or tints[i] != [1.0, 1.0, 1.0]:
            raise ValueError("instance %d is moved: it takes no density_scale or tint of its own" % i)
        scale[i] = 0.0
    if given:
        near, far = batch["near_inst"], batch["far_inst"]
    elif RTs is not None:
        near, far, _ = ops.sample_rays_in_bbox_list(RTs, batch["rays_o"], batch["viewdirs"])
    else:
        near = far = torch.zeros(0, batch["rays_o"].shape[0], device=batch["rays_o"].device)

    def once():
        layers = instance_layers(model, batch, RTs, moves, chunk) if moved else None
        if layers is not None:
            layers = {k: layers[k] for k in ("key", "rgb", "acc", "depth")}
        res = model.render_edited(batch, near, far, density_scale=scale, tint=tints, layers=layers, chunk=chunk)[1]
        out = dict(rgb=res[0], depth=res[5], acc=res[3], bg_lambda=res[4])
        if layers is not None:
            out["visibility"] = res[6]
        return out
    return _render_guarded(model, batch, once, check, on_range)


@torch.no_grad()
def render_decomposed_rays(model, batch, RTs=None, chunk=1024, check=True, on_range="retry_f32"):
    """Decomposed frame of a NeRF_TP module: the fine level of `model.render_decomposed` on every ray of `batch` in one library
    call, with the reference chunk size passed down.  The per-instance intervals are batch["near_inst"] / batch["far_inst"] when
    present, else they are computed from `RTs` with ops.sample_rays_in_bbox_list; with neither, K = 0.  Returns dict(rgb (R,3),
    depth (R,), acc (R,), fg_rgb, bg_rgb (R,3)) - rgb / depth bitwise render_rays_test's - plus
        layer_rgb (K+1,R,3)  the colour each instance contributes to the frame as it is seen IN the scene (occluded by whatever
                             stands in front of it); slot K is everything else, bg_lambda * bg_rgb included (fg + lambda bg, the
                             merge's own two fp32 operations: with K = 0 it is `rgb`, bitwise).  The layers add up to `rgb`;
        layer_acc (K+1,R)    the mattes (inside-sphere weight per slot; they add up to `acc`);
        layer_depth (K+1,R)  the slot's expected ray parameter, sum w t / sum w where layer_acc > 0, else 0;
        instance_id (R,)     int32, the instance that holds the largest share of the ray's weight if that share is at least the
                             share of everything else (the outside-sphere half included), else -1;
    and `target` / `instance_mask` passed through.  Everything runs inside one guarded render (check / on_range: the flag read,
    range-guard retry and latch of render_rays_test)."""
    if not isinstance(model, models.NeRF_TP):
        raise TypeError("render_decomposed_rays renders NeRF_TP modules, got %r" % type(model))
    if "near_inst" in batch and "far_inst" in batch:
        near, far = batch["near_inst"], batch["far_inst"]
    elif RTs is not None:
        from . import ops
        near, far, _ = ops.sample_rays_in_bbox_list(RTs, batch["rays_o"], batch["viewdirs"])
    else:
        near = far = torch.zeros(0, batch["rays_o"].shape[0], device=batch["rays_o"].device)

    def once():
        res = model.render_decomposed(batch, near, far, chunk=chunk)[1]
        dec = res[6]
        K = dec["acc"].shape[0] - 1
        layer_rgb = dec["rgb"].clone()
        layer_rgb[K] = dec["rgb"][K] + res[4] * res[2]
        seen = dec["acc"] > 0
        layer_depth = torch.where(seen, dec["depth"] / torch.where(seen, dec["acc"], torch.ones_like(dec["acc"])), torch.zeros_like(dec["acc"]))
        return dict(rgb=res[0], depth=res[5], acc=res[3], fg_rgb=res[1], bg_rgb=res[2], layer_rgb=layer_rgb, layer_acc=dec["acc"],
                    layer_depth=layer_depth, instance_id=dec["id"])
    return _render_guarded(model, batch, once, check, on_range)


def _march_result(model, fine, kept, survivors=None):
    """The dict of the skipping / marching frame wrappers from the fine level tuple and the call's device counters: rgb, depth, acc,
    `kept_fraction` (kept[0:2] over the inside-sphere samples of each level), with a 4-entry `kept` also `kept_fraction_outside`
    (kept[2:4] over the same counts), with `survivors` also `culled_fraction`.  No host read, no sync: the scalar divisors travel as
    kernel arguments."""
    R = fine[0].shape[0]
    n0 = model.num_coarse_samples + 1
    per = (float(max(R * n0, 1)), float(max(R * (n0 + model.num_fine_samples), 1)))
    kept = kept.double()
    out = dict(rgb=fine[0], depth=fine[5], acc=fine[3], kept_fraction=torch.stack([kept[0] / per[0], kept[1] / per[1]]))
    if kept.shape[0] == 4:
        out["kept_fraction_outside"] = torch.stack([kept[2] / per[0], kept[3] / per[1]])
    if survivors is not None:
        out["culled_fraction"] = 1.0 - survivors.double() / float(max(R, 1))
    return out


@torch.no_grad()
def render_skipping_rays(model, batch, chunk=1024, check=True, on_range="retry_f32"):
    """Frame of a NeRF_TP module with empty space skipped: the fine level of `model.render_skipping` (which needs an occupancy
    grid: `model.build_occupancy` / `model.set_occupancy`) on every ray of `batch` in one library call, with the reference chunk
    size passed down - the place of the reference's chunk loop.  Returns dict(rgb (R,3), depth (R,), acc (R,)) plus
    `kept_fraction`, a (2,) float64 DEVICE tensor: the share of inside-sphere samples evaluated at level 0 and level 1 (reading it
    synchronises, the call does not), and `target` / `instance_mask` passed through.  With an all-ones grid rgb / depth are bitwise
    render_rays_test's.  check / on_range: the flag read, range-guard retry and latch of render_rays_test (the same code path)."""
    if not isinstance(model, models.NeRF_TP):
        raise TypeError("render_skipping_rays renders NeRF_TP modules, got %r" % type(model))

    def once():
        res = model.render_skipping(batch, chunk=chunk)
        return _march_result(model, res[1], model.last_skip_kept)
    return _render_guarded(model, batch, once, check, on_range)


@torch.no_grad()
def render_terminating_rays(model, batch, eps, chunk=1024, segment=64, coarse=False, check=True, on_range="retry_f32"):
    """Frame of a NeRF_TP module with early ray termination: the fine level of `model.render_terminating(batch, eps, ...)` on every
    ray of `batch` in one library call, with the reference chunk size passed down.  Returns dict(rgb (R,3), depth (R,), acc (R,))
    plus `kept_fraction`, a (2,) float64 DEVICE tensor - the share of inside-sphere samples evaluated at level 0 and level 1 - and
    `culled_fraction`, a float64 DEVICE scalar - the share of rays whose outside-sphere half did not run (reading either
    synchronises, the call does not) - and `target` / `instance_mask` passed through.  With eps = 0 rgb / depth are bitwise
    render_rays_test's.  check / on_range: the flag read, range-guard retry and latch of render_rays_test (the same code path)."""
    if not isinstance(model, models.NeRF_TP):
        raise TypeError("render_terminating_rays renders NeRF_TP modules, got %r" % type(model))

    def once():
        res = model.render_terminating(batch, eps, chunk=chunk, segment=segment, coarse=coarse)
        return _march_result(model, res[1], model.last_terminate_kept, model.last_terminate_survivors)
    return _render_guarded(model, batch, once, check, on_range)


@torch.no_grad()
def render_accelerated_rays(model, batch, eps, chunk=1024, segment=64, coarse=False, check=True, on_range="retry_f32"):
    """Frame of a NeRF_TP module with empty space skipped AND early ray termination: the fine level of
    `model.render_accelerated(batch, eps, ...)` on every ray of `batch` in one library call, with the reference chunk size passed
    down.  Returns dict(rgb (R,3), depth (R,), acc (R,)) plus `kept_fraction`, a (2,) float64 DEVICE tensor - the share of
    inside-sphere samples evaluated at level 0 and level 1 - and `culled_fraction`, a float64 DEVICE scalar - the share of rays whose
    outside-sphere half did not run (reading either synchronises, the call does not) - and `target` / `instance_mask` passed through.
    Without a grid it is render_terminating_rays; with eps = 0, render_skipping_rays.  check / on_range: the flag read, range-guard
    retry and latch of render_rays_test (the same code path)."""
    if not isinstance(model, models.NeRF_TP):
        raise TypeError("render_accelerated_rays renders NeRF_TP modules, got %r" % type(model))

    def once():
        res = model.render_accelerated(batch, eps, chunk=chunk, segment=segment, coarse=coarse)
        return _march_result(model, res[1], model.last_accel_kept, model.last_accel_survivors)
    return _render_guarded(model, batch, once, check, on_range)


@torch.no_grad()
def render_marching_rays(model, batch, eps, chunk=1024, segment=64, coarse=False, outside=True, grid=True, check=True,
                         on_range="retry_f32"):
    """Frame of a NeRF_TP module with early ray termination inside AND outside the sphere: the fine level of
    `model.render_marching(batch, eps, ...)` on every ray of `batch` in one library call, with the reference chunk size passed down.
    Returns dict(rgb (R,3), depth (R,), acc (R,)) plus `kept_fraction`, a (2,) float64 DEVICE tensor - the share of inside-sphere
    samples evaluated at level 0 and level 1 - `kept_fraction_outside`, the same for the outside-sphere samples (over ALL rays: a
    culled ray keeps none), and `culled_fraction`, a float64 DEVICE scalar - the share of rays whose outside-sphere half did not run
    (reading any of them synchronises, the call does not) - and `target` / `instance_mask` passed through.  outside=False is
    render_accelerated_rays (grid=True) or render_terminating_rays (grid=False); with eps = 0 and no grid rgb / depth are bitwise
    render_rays_test's.  check / on_range: the flag read, range-guard retry and latch of render_rays_test (the same code path)."""
    if not isinstance(model, models.NeRF_TP):
        raise TypeError("render_marching_rays renders NeRF_TP modules, got %r" % type(model))

    def once():
        res = model.render_marching(batch, eps, chunk=chunk, segment=segment, coarse=coarse, outside=outside, grid=grid)
        return _march_result(model, res[1], model.last_march_kept, model.last_march_survivors)
    return _render_guarded(model, batch, once, check, on_range)


@torch.no_grad()
def render_frame_sharded(model, batch, world, rank, chunk=1024, white_bkgd=False, near=0.2, far=3.0, group=None,
                         gather=True, train_frac=1.0, n_rays=None, out=None, reuse=False, check=True, always_gather=False,
                         info=None, image_width=None):
    """This rank renders its contiguous range of whole chunks; `gather=True` reassembles
    the full (R,5) = (rgb, depth, acc) frame on every rank with one all-gather.
    `batch` holds the whole frame's rays, or - with n_rays = R given - only this rank's shard
    (rays [shard_bounds(R, world, rank)), e.g. from ops.get_ray_directions_and_rays(ray_range=...)).
    The gathered frame is a fresh tensor unless `out=` / `reuse=True` are given (parallel.gather_tiles).
    always_gather: run the collective at world == 1 too (a one-rank process group: the RCCL call path of the N-GPU job
    on a one-GPU box; bench.py under `torchrun --nproc-per-node 1`).
    info: an optional dict that receives `precision_used` = the arithmetic THIS rank's shard was rendered in ("f16x3" /
    "f32": a range-guard retry, see render_rays_test) and, when the frame is gathered over more than one rank,
    `precision_by_rank` (one extra 4-byte all-gather, only when `info` is given): a frame whose ranks mixed arithmetics
    says so instead of hiding it in the gathered tile."""
    # rays_o defines the rows of the batch: checked before `_slice` cuts every tensor to the shard's rows, which would make a
    # longer tensor of another frame pass for this frame's
    first = ray_rows(batch, tuple(k for k in ("rays_o", "rays_d", "viewdirs") if k in batch), on_device=False)[0]
    if "radii" in batch:
        dense(batch["radii"], "radii", radii_shapes(first.shape[0]), on_device=False)
    if n_rays is None:
        R = batch["rays_o"].shape[0]
        lo, hi = shard_bounds(R, world, rank, unit=chunk)
        mine = _slice(batch, lo, hi)
    else:
        R = int(n_rays)
        lo, hi = shard_bounds(R, world, rank, unit=chunk)
        assert batch["rays_o"].shape[0] == hi - lo, "batch must hold exactly this rank's shard"
        mine = batch
    part = render_rays_test(model, mine, chunk, white_bkgd, near, far, train_frac, check=check, image_width=image_width, first_ray=lo)
    tile = torch.cat([part["rgb"], part["depth"][:, None], part["acc"][:, None]], dim=1)
    used = part.get("precision_used") or getattr(model, "last_precision_used", None) or model.precision or model.default_precision
    if info is not None:
        info["precision_used"] = used
    if not gather or (world == 1 and not always_gather):
        return tile
    if info is not None and world > 1:
        import torch.distributed as dist
        mine_p = torch.tensor([1 if used == "f32" else 0], dtype=torch.int32, device=tile.device)
        every = torch.empty(world, dtype=torch.int32, device=tile.device)
        dist.all_gather_into_tensor(every, mine_p, group=group)
        info["precision_by_rank"] = ["f32" if int(x) else "f16x3" for x in every.tolist()]
    return gather_tiles(tile, R, world, unit=chunk, group=group, out=out, reuse=reuse)


def psnr(pred, gt):
    """-10 ln(mse)/ln 10 on images clipped to [0,1] (models/interface.py:53-61)."""
    mse = torch.mean((torch.clip(pred, 0, 1) - torch.clip(gt, 0, 1)) ** 2)
    return float("inf") if float(mse) == 0.0 else float(-10.0 * torch.log(mse) / math.log(10))
