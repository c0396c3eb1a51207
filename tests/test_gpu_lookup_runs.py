"""GPU: the feature lookups forward and their run-merged scatter backward (k_gather_bwd_runs, k_map_gather_bwd_runs) on RAY-ORDERED
points, where the merge really happens.  A 16-lane group of the backward walks 16 consecutive rows (view-major: row = v P + p) and
keeps one texel per tap slot in registers, flushing when it changes.  Uniformly random points - what the other direct tests draw -
practically never put two consecutive rows on one texel, so the accumulate-across-rows branch, the flush inside a run, a run that
crosses a view boundary and the short last run were only reached through whole training steps at loose bounds.

Points: 40 strided rays x 49 samples over cases.small_scene() (P = 1960 is no multiple of 16: runs cross the view boundaries), one
ray whose samples all sit at one point (49 rows on one texel), one ray exactly on texel centres of view 0's xz plane (three tap
weights exactly zero; view 0 has the identity pose so that its camera-frame coordinates are the world coordinates bit for bit),
one ray off every plane.  Truth: fp64 autograd through oracle.gather; bound 1e-5 x max(1, largest |fp64 entry|) as in
test_gpu_training.py::test_gather_forward_and_backward.  Bitwise repeatability of these gradients is NOT asserted: the scatter
adds with float atomics, whose order differs from run to run."""
import numpy as np
import pytest
import torch

import alongray_cases as A
import cases
import oracle
from conftest import record_parity
from neo360_amd import models, training

gpu = pytest.mark.gpu          # the check of the points themselves needs no device
DEV = "cuda"
RAYS, SAMPLES = 40, 49
MAPS = ("plane_xz", "plane_xy", "plane_yz", "latent")


def _exact_centres(size):
    """fp32 grid coordinates g whose pixel ((g + 1) / 2) * (size - 1) is an integer in fp32 arithmetic, interior texels only."""
    out = []
    for k in range(1, size - 1):
        g = np.float32(2.0 * k / (size - 1) - 1.0)
        if ((g + np.float32(1.0)) / np.float32(2.0)) * np.float32(size - 1) == np.float32(k):
            out.append(float(g))
    return out


def ray_ordered_points():
    rays = cases.strided_rays(RAYS)
    far, _ = oracle.rays.sphere_exit_depth(rays["rays_o"], rays["rays_d"])
    t = (torch.linspace(0.05, 0.95, SAMPLES)[None, :] * far).contiguous()
    pts = oracle.sampling.points_on_rays(t, rays["rays_o"], rays["rays_d"]).clone()          # (RAYS, SAMPLES, 3)
    pts[7] = pts[7, 20]                                                                       # one point, 49 times
    xs, zs = _exact_centres(cases.PLANE_HW[1]), _exact_centres(cases.PLANE_HW[0])
    assert len(xs) >= 3 and len(zs) >= 3
    for i in range(SAMPLES):                                                                  # texel centres of view 0's xz plane,
        pts[11, i] = torch.tensor([xs[(i // 6) % len(xs)], 0.3, zs[(i // 12) % len(zs)]])     # each held for a few rows
    pts[13] = pts[13] * 4.0                                                                   # off every plane
    return pts.reshape(-1, 3).contiguous()


def batch_for(nv):
    batch = cases.neo_batch(cases.strided_rays(8), nv)
    batch["src_poses"] = batch["src_poses"].clone()
    batch["src_poses"][0] = torch.eye(4)                  # view 0: camera frame = world frame, exactly
    return batch


def consecutive_rows_sharing_a_cell(pts, batch, hw, latent=False):
    """Fraction of the consecutive (view-major) row pairs whose first tap is the same texel of the same view."""
    cam = oracle.gather.world_to_camera(pts.double(), batch["src_poses"].double())          # (NV, P, 3)
    H, W = hw
    if latent:
        f = batch["src_focal"][0].double() * torch.tensor([1.0, -1.0], dtype=torch.float64)
        uv = oracle.gather.project(cam, f, batch["src_c"][0].double())
        g = uv * (oracle.gather.latent_scaling(H, W).double() / torch.tensor(cases.IMG_WH, dtype=torch.float64)) - 1.0
    else:
        g = cam[..., [0, 2]]
    cell = torch.stack([torch.floor((g[..., 0] + 1) / 2 * (W - 1)), torch.floor((g[..., 1] + 1) / 2 * (H - 1))], dim=-1)
    view = torch.arange(cam.shape[0], dtype=torch.float64)[:, None, None].expand(-1, cam.shape[1], 1)
    key = torch.cat([view, cell], dim=-1).reshape(-1, 3)
    return float((key[1:] == key[:-1]).all(dim=-1).double().mean())


def _net(nv, scene):
    net = models.NeRF_TP(num_coarse_samples=32, num_fine_samples=64, num_src_views=nv).to(DEV)
    net.set_scene(*(scene[k].to(DEV) for k in MAPS), scene["image_wh"])
    return net


def _check(label, got, ref64, ref32):
    checks = {k: A.worst_entry(got[k], ref64[k], A.LOOKUP * A.scale_of(ref64[k]), ref32[k]) for k in got}
    record_parity("alongray_sweep/lookup_runs/" + label, **A.summarize(checks))
    A.assert_inside(checks, label)


def test_the_points_make_runs():
    """At least half of the consecutive rows share a plane cell: the test cannot silently stop exercising the merge."""
    pts = ray_ordered_points()
    assert pts.shape[0] == RAYS * SAMPLES and pts.shape[0] % 16 != 0
    for nv in (1, 3, 5):
        batch = batch_for(nv)
        plane = consecutive_rows_sharing_a_cell(pts, batch, cases.PLANE_HW)
        lat = consecutive_rows_sharing_a_cell(pts, batch, cases.LATENT_HW, latent=True)
        print("NV = %d: %.0f %% of the consecutive rows share a plane cell, %.0f %% a latent cell" % (nv, 100 * plane, 100 * lat))
        assert plane >= 0.5, (nv, plane)
        assert lat >= 0.1, (nv, lat)          # fewer: a step along a ray is about a latent texel, and view 0's identity pose projects widely


def _oracle_features(pts, scene, batch, dtype, planes_only):
    c = lambda x: x.to(dtype)
    with torch.enable_grad():
        cm = {k: c(scene[k]).clone().requires_grad_(True) for k in MAPS}
        world = oracle.gather.triplane_features(c(pts), cm["plane_xz"], cm["plane_xy"], cm["plane_yz"], c(batch["src_poses"]))
        outs, ups = [world], [c(batch["up_world"])]
        if not planes_only:
            outs.append(oracle.gather.pixel_aligned_features(c(pts), cm["latent"], c(batch["src_poses"]), c(batch["src_focal"]),
                                                             c(batch["src_c"]), scene["image_wh"]))
            ups.append(c(batch["up_local"]))
        loss = sum((o.reshape(u.shape) * u).sum() for o, u in zip(outs, ups))
        names = MAPS[:3] if planes_only else MAPS
        grads = torch.autograd.grad(loss, [cm[k] for k in names])
    res = dict(world=world.detach())
    if not planes_only:
        res["local"] = outs[1].detach()
    res.update({"g_" + k: g for k, g in zip(names, grads)})
    return res


@gpu
@pytest.mark.parametrize("nv", [1, 3, 5])
def test_gather_features_and_planes_on_ray_ordered_points(nv):
    scene = cases.small_scene(nv=nv)
    pts = ray_ordered_points()
    batch = batch_for(nv)
    gen = torch.Generator().manual_seed(40 + nv)
    batch["up_world"] = torch.randn(nv * pts.shape[0], 128, generator=gen)
    batch["up_local"] = torch.randn(nv * pts.shape[0], 512, generator=gen)
    gbatch = {k: v.to(DEV) for k, v in batch.items()}
    net = _net(nv, scene)
    for planes_only in (False, True):
        ref64 = _oracle_features(pts, scene, batch, torch.float64, planes_only)
        ref32 = _oracle_features(pts, scene, batch, torch.float32, planes_only)
        with torch.enable_grad():
            gm = {k: scene[k].to(DEV).clone().requires_grad_(True) for k in MAPS}
            if planes_only:
                world = training.gather_planes(net, pts.to(DEV), gm["plane_xz"], gm["plane_xy"], gm["plane_yz"], gm["latent"], gbatch)
                loss = (world * gbatch["up_world"]).sum()
                got = dict(world=world.detach())
            else:
                world, local = training.gather_features(net, pts.to(DEV), gm["plane_xz"], gm["plane_xy"], gm["plane_yz"], gm["latent"], gbatch)
                loss = (world * gbatch["up_world"]).sum() + (local * gbatch["up_local"]).sum()
                got = dict(world=world.detach(), local=local.detach())
            names = MAPS[:3] if planes_only else MAPS
            grads = torch.autograd.grad(loss, [gm[k] for k in names])
        got.update({"g_" + k: g for k, g in zip(names, grads)})
        _check("%s_nv%d" % ("gather_planes" if planes_only else "gather_features", nv), got, ref64, ref32)
    net.close()


@gpu
@pytest.mark.parametrize("nv", [1, 3, 5])
def test_gather_map_on_ray_ordered_points(nv):
    """A caller-owned channels-last map at the latent's taps: whole maps of width 256 and 128, and columns [64, 320) of a 384-wide
    map (row pitch 384; the gradient outside the slice stays zero)."""
    scene = cases.small_scene(nv=nv)
    pts = ray_ordered_points()
    batch = batch_for(nv)
    gbatch = {k: v.to(DEV) for k, v in batch.items()}
    net = _net(nv, scene)
    Hf, Wf = cases.LATENT_HW
    for width, col, take in ((256, None, None), (128, None, None), (384, 64, 256)):
        gen = torch.Generator().manual_seed(60 + nv + width)
        gmap = torch.randn(nv * Hf * Wf, width, generator=gen) * 0.5
        C = take if col is not None else width
        up = torch.randn(nv * pts.shape[0], C, generator=gen)

        def reference(dtype):
            with torch.enable_grad():
                m = gmap.to(dtype).clone().requires_grad_(True)
                sl = m[:, col:col + take] if col is not None else m
                nchw = sl.reshape(nv, Hf, Wf, C).permute(0, 3, 1, 2)
                out = oracle.gather.pixel_aligned_features(pts.to(dtype), nchw, batch["src_poses"].to(dtype), batch["src_focal"].to(dtype),
                                                           batch["src_c"].to(dtype), scene["image_wh"])
                (g,) = torch.autograd.grad((out * up.to(dtype)).sum(), m)
            return dict(out=out.detach(), g_map=g)

        ref64, ref32 = reference(torch.float64), reference(torch.float32)
        with torch.enable_grad():
            m = gmap.to(DEV).requires_grad_(True)
            out = training.gather_map(net, m, pts.to(DEV), gbatch, col=col, width=take)
            (g,) = torch.autograd.grad((out * up.to(DEV)).sum(), m)
        if col is not None:
            assert bool((g[:, :col] == 0).all()) and bool((g[:, col + take:] == 0).all())
        _check("gather_map_w%d%s_nv%d" % (width, "_slice" if col is not None else "", nv), dict(out=out.detach(), g_map=g), ref64, ref32)
    net.close()
