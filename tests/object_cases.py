"""Shared inputs of the object-render tests (tests/test_objects_cpu.py, tests/test_gpu_objects.py).

Scene: cases.small_scene() seen by cases.strided_rays(n), synth.nerf_tp_state(0) with both foreground density biases raised by
+6 (so that a short march through a box accumulates a visible opacity), and two oriented boxes in the reference's `RTs` format
(models/neo360/helper.py:348-373: R, T = box-to-world rotation / translation, s = the (2,3) corner bounds in the box frame):

    box A   R = rot_z(0.4) . rot_x(-0.3)   T = (0.05, -0.05, 0)     half-extents (0.18, 0.12, 0.15)
    box B   R = identity                   T = (-0.25, 0.2, 0.05)   0.1 cube

Near / far come from the CPU oracle (oracle.rays.sample_rays_in_bbox), so nothing here depends on the GPU box kernel.

The CPU oracle of the object render composes the existing oracle functions with the object interval in place of the sphere
interval: sampling.neo_fg_level0(near = max(near_obj, 1e-4), far = far_obj) -> neo360.region_eval(fg_coarse_mlp) ->
compositing.neo_composite(in_sphere, t_far = far_obj, white_bkgd) -> sampling.neo_fg_level1 -> region_eval(fg_fine_mlp) ->
neo_composite.  It runs on ALL rays of a chunk (the view-direction tiling, quirk Q1, needs the whole chunk); missed rays are
marched through a dummy interval and are to be ignored by the caller.
"""
import math

import numpy as np
import torch

import cases
import oracle
from neo360_amd import synth

BIAS = 6.0
NEAR = 1e-4          # neo360/model.py:277
PER_RAY = ("rays_o", "rays_d", "viewdirs")


def _rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def _bounds(h):
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (3,))
    return np.stack([-h, h])


BOX_A = dict(R=_rot_z(0.4) @ _rot_x(-0.3), T=np.array([0.05, -0.05, 0.0]), s=_bounds((0.18, 0.12, 0.15)))
BOX_B = dict(R=np.eye(3), T=np.array([-0.25, 0.2, 0.05]), s=_bounds(0.1))


def rts(*boxes):
    """The reference's RTs dict of these boxes (default: A and B)."""
    boxes = boxes or (BOX_A, BOX_B)
    return dict(R=[b["R"] for b in boxes], T=[b["T"] for b in boxes], s=[b["s"] for b in boxes])


def state():
    st = synth.nerf_tp_state(0)
    for k in ("fg_coarse_mlp.density_layer.bias", "fg_fine_mlp.density_layer.bias"):
        st[k] = st[k] + BIAS
    return st


def bounds_of(rays, *boxes):
    """near_obj, far_obj (R,) float32 and the hit mask (R,) of CPU rays, from the CPU oracle of sample_rays_in_bbox."""
    near, far, mask, _ = oracle.rays.sample_rays_in_bbox(rts(*boxes), rays["rays_o"].double().numpy(), rays["viewdirs"].double().numpy())
    return near.reshape(-1), far.reshape(-1), mask.reshape(-1)


def hit_rule(near, far):
    """The entry point's hit rule on CPU tensors: lo = max(near, 1e-4), hi = far; hit iff both finite and hi > lo."""
    lo = torch.where(near > NEAR, near, torch.full_like(near, NEAR))
    hit = torch.isfinite(near) & torch.isfinite(far) & (far > lo)
    return lo, far, hit


_BATCHES = {}


def batch(n, *boxes):
    """CPU batch of cases.strided_rays(n) with the reference's near_obj / far_obj keys (R,1), cached: (batch, hit mask)."""
    key = (n, tuple(id(b) for b in boxes))
    if key not in _BATCHES:
        b = cases.neo_batch(cases.strided_rays(n))
        near, far, mask = bounds_of(b, *boxes)
        b["near_obj"], b["far_obj"] = near.reshape(-1, 1), far.reshape(-1, 1)
        _BATCHES[key] = (b, mask)
    b, mask = _BATCHES[key]
    return dict(b), mask.clone()


def frame_batch(H=48, W=64):
    """The H x W frame of cases.crop_rays with the bounds of both boxes."""
    b = cases.neo_batch(cases.crop_rays(H, W))
    near, far, mask = bounds_of(b)
    b["near_obj"], b["far_obj"] = near.reshape(-1, 1), far.reshape(-1, 1)
    return b, mask


def oracle_render(params, b, near_obj, far_obj, n_coarse, n_fine, white_bkgd=True, chunk=None, t1=None, scene=None):
    """CPU oracle of render_objects on ALL rays of `b` (CPU tensors), chunk by chunk.  t1: level-1 sample rows (R, N1) to USE
    instead of resampling.  Returns dict(hit, t0, t1, rgb0, acc0, depth0, rgb1, acc1, depth1); only rows with `hit` mean anything
    (a missed ray is marched through the dummy interval [1e-4, 1])."""
    scene = scene if scene is not None else cases.small_scene()
    near_obj, far_obj = near_obj.reshape(-1).float(), far_obj.reshape(-1).float()
    lo, hi, hit = hit_rule(near_obj, far_obj)
    lo = torch.where(hit, lo, torch.full_like(lo, NEAR))
    hi = torch.where(hit, hi, torch.ones_like(hi))
    R = lo.shape[0]
    chunk = chunk or R
    parts = []
    for i in range(0, R, chunk):
        part = {k: (v[i:i + chunk] if k in PER_RAY else v) for k, v in b.items()}
        o, d = part["rays_o"], part["rays_d"]
        near, far = lo[i:i + chunk, None], hi[i:i + chunk, None]
        t0, _ = oracle.sampling.neo_fg_level0(o, d, n_coarse, near, far)
        rgb, sigma = oracle.neo360.region_eval(params, "fg_coarse_mlp.", part, scene, t0, True)
        c0, acc0, w0, _, depth0 = oracle.compositing.neo_composite(rgb, sigma, t0, d, True, far, white_bkgd)
        if t1 is not None:
            tf = t1[i:i + chunk]
        else:
            mid = 0.5 * (t0[..., 1:] + t0[..., :-1])
            tf, _ = oracle.sampling.neo_fg_level1(mid, w0[..., 1:-1], o, d, t0, n_fine)
        rgb, sigma = oracle.neo360.region_eval(params, "fg_fine_mlp.", part, scene, tf, True)
        c1, acc1, _, _, depth1 = oracle.compositing.neo_composite(rgb, sigma, tf, d, True, far, white_bkgd)
        parts.append(dict(t0=t0, t1=tf, rgb0=c0, acc0=acc0.reshape(-1), depth0=depth0.reshape(-1), rgb1=c1, acc1=acc1.reshape(-1),
                          depth1=depth1.reshape(-1)))
    out = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    out["hit"] = hit
    return out
