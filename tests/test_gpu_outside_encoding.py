"""GPU: the outside-sphere point evaluator's encoding schedule (csrc/pe_schedule.h, k_tp_mlp_hpp<4>) against the oracle.

Outside the unit sphere k_tp_mlp_hpp<4> encodes 1/r once per 64-point tile and the camera-frame x, y, z once per view, the pairs
spread 8 / 8 / 7 / 7 over the four waves; the closing block reads each row's launch point from LDS and the work list's group bits
come from the wave that computed a map's weights.  `net.eval_mlp` of slots 2 and 3 (outside coarse / fine) against
`oracle.neo360.region_eval` at the stage bound 2e-5 (tests/test_gpu_neo360_stages.py), on `cases.small_scene()`:

* shapes: 7 rays x 129 samples (903 points: a ragged last tile) and 5 x 385 (the R % G rows that stay ray-major beside one quad);
* sample rows: one shared row for all rays (coarse-style) and per-ray descending rows (fine-style); rows that hold s = 0 exactly and
  s = 1 - 2^-20 (the encoding's arguments at their extremes: 1/r = 0, and 512 (1 - 2^-20) at octave 9);
* 1 and 3 source views (the view loop's length); the default pre-projection (mode 3) and f16x3-pp2, where slots 0 / 1 run
  k_tp_mlp_hpp<3>, whose encoding is untouched - checked inside the sphere as well;
* a replicated ray: 64 identical rays x 129 samples - every ray's row of the result must be the same bits, whichever tile row and
  wave computed it, at 0 / 4 / 16 rays per group;
* group widths: one launch at 0 / 4 / 16 rays per group gives bitwise-equal arrays.
"""
import pytest
import torch

import cases
import oracle
from conftest import max_abs
from neo360_amd import models, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 2e-5
OUTSIDE = ((2, "bg_coarse_mlp."), (3, "bg_fine_mlp."))
INSIDE = ((0, "fg_coarse_mlp."), (1, "fg_fine_mlp."))
SHAPES = {"ragged-7x129": (7, 129), "leftover-5x385": (5, 385)}
WIDTHS = (0, 4, 16)
_NETS, _ORACLE = {}, {}


def _net(nv, variant):
    if (nv, variant) not in _NETS:
        net = models.NeRF_TP(num_coarse_samples=128, num_fine_samples=256, num_src_views=nv).to(DEV)
        net.precision = "f16x3"
        net.load_state_dict(synth.nerf_tp_state(0))
        sc = cases.small_scene(nv=nv)
        net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV), sc["image_wh"],
                      preproject={"default": None, "f16x3-pp2": 2}[variant])
        _NETS[(nv, variant)] = (net, sc)
    return _NETS[(nv, variant)]


def _rows(style, R, N):
    """(R, N) descending inverse radii."""
    if style == "shared":
        return torch.linspace(0.99, 0.01, N)[None, :].expand(R, N).contiguous()
    if style == "per-ray":
        g = torch.Generator().manual_seed(1000 * R + N)
        return torch.sort(torch.rand(R, N, generator=g) * 0.98 + 0.01, dim=1, descending=True)[0].contiguous()
    assert style == "edges"
    s = torch.linspace(1.0, 0.0, N)[None, :].expand(R, N).clone()
    s[:, 0] = 1.0 - 2.0 ** -20
    s[:, -1] = 0.0
    assert float(s[0, 0]) < 1.0 and float(s[0, -1]) == 0.0 and bool((s[:, 1:] < s[:, :-1]).all())
    return s


def _want(nv, prefix, key, batch, scene, tv, inside, far_c):
    """The oracle's (rgb, sigma) - the same for every kernel variant: evaluated once per session."""
    k = (nv, prefix, key)
    if k not in _ORACLE:
        _ORACLE[k] = oracle.neo360.region_eval(synth.nerf_tp_state(0), prefix, batch, scene, tv, inside, far_c)
    return _ORACLE[k]


def _check(net, nv, scene, batch, slot, prefix, key, tv, inside, far_c, far_g):
    got = net.eval_mlp(slot, {k: v.to(DEV) for k, v in batch.items()}, tv.to(DEV), far=far_g).cpu()
    rgb, sigma = _want(nv, prefix, key, batch, scene, tv, inside, far_c)
    e_rgb, e_sigma = max_abs(got[..., :3], rgb), max_abs(got[..., 3:], sigma)
    print("%s slot %d nv %d: max|rgb err| %.2e  max|sigma err| %.2e" % (key, slot, nv, e_rgb, e_sigma))
    assert e_rgb < BOUND and e_sigma < BOUND, (key, slot, nv, e_rgb, e_sigma)
    return got


def _far(batch):
    far_c, _ = oracle.rays.sphere_exit_depth(batch["rays_o"], batch["rays_d"])
    far_g, ok = ops.intersect_sphere(batch["rays_o"].to(DEV), batch["rays_d"].to(DEV))
    assert bool(ok.all())
    return far_c, far_g


@pytest.mark.parametrize("variant", ["default", "f16x3-pp2"])
@pytest.mark.parametrize("nv", [1, 3], ids=["1view", "3views"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_outside_slots_against_the_oracle(shape, nv, variant):
    R, N = SHAPES[shape]
    net, scene = _net(nv, variant)
    batch = cases.neo_batch(cases.strided_rays(R), nv=nv)
    far_c, far_g = _far(batch)
    for style in ("shared", "per-ray"):
        tv = _rows(style, R, N)
        for slot, prefix in OUTSIDE:
            _check(net, nv, scene, batch, slot, prefix, (shape, style), tv, False, far_c, far_g)
    assert net._context(torch.device(DEV)).poll_flags() == 0


@pytest.mark.parametrize("variant", ["default", "f16x3-pp2"])
def test_edge_values_of_s(variant):
    R, N, nv = 7, 129, 3
    net, scene = _net(nv, variant)
    batch = cases.neo_batch(cases.strided_rays(R), nv=nv)
    far_c, far_g = _far(batch)
    tv = _rows("edges", R, N)
    for slot, prefix in OUTSIDE:
        got = _check(net, nv, scene, batch, slot, prefix, ("edges",), tv, False, far_c, far_g)
        assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("nv", [1, 3], ids=["1view", "3views"])
def test_inside_slots_of_pp2_are_unchanged_against_the_oracle(nv):
    """f16x3-pp2 runs k_tp_mlp_hpp<3> inside the sphere: three coordinates, the encoding of every view as before."""
    R, N = SHAPES["ragged-7x129"]
    net, scene = _net(nv, "f16x3-pp2")
    batch = cases.neo_batch(cases.strided_rays(R), nv=nv)
    far_c, far_g = _far(batch)
    tv = torch.linspace(0.02, 0.98, N)[None, :] * far_c.reshape(-1, 1)
    for slot, prefix in INSIDE:
        _check(net, nv, scene, batch, slot, prefix, ("inside",), tv, True, far_c, far_g)


@pytest.mark.parametrize("variant", ["default", "f16x3-pp2"])
def test_replicated_ray_gives_the_same_bits_in_every_tile_row_and_wave(variant):
    R, N, nv = 64, 129, 3
    net, scene = _net(nv, variant)
    one = cases.neo_batch(cases.strided_rays(1), nv=nv)
    batch = {k: (v if k.startswith("src_") else v.expand(R, *v.shape[1:]).contiguous()) for k, v in one.items()}
    far_c, far_g = _far(batch)
    ctx = net._context(torch.device(DEV))
    try:
        for style in ("shared", "edges"):
            tv = _rows(style, R, N)
            for slot, prefix in OUTSIDE:
                first = None
                for width in WIDTHS:
                    ctx.set_tp_quad(width)
                    got = net.eval_mlp(slot, {k: v.to(DEV) for k, v in batch.items()}, tv.to(DEV), far=far_g)
                    assert torch.equal(got, got[:1].expand_as(got)), (style, slot, width, "rays of one launch differ",
                                                                      float((got - got[:1]).abs().max()))
                    first = got if first is None else first
                    assert torch.equal(got, first), (style, slot, width, "differs from ray-major")
                rgb, sigma = _want(nv, prefix, ("one ray", style), one, scene, tv[:1], False, far_c[:1])
                assert max_abs(first[:1, :, :3].cpu(), rgb) < BOUND and max_abs(first[:1, :, 3:].cpu(), sigma) < BOUND, (style, slot)
    finally:
        ctx.set_tp_quad(None)


@pytest.mark.parametrize("variant", ["default", "f16x3-pp2"])
@pytest.mark.parametrize("nv", [1, 3], ids=["1view", "3views"])
def test_group_widths_are_bitwise_equal(nv, variant):
    net, _ = _net(nv, variant)
    ctx = net._context(torch.device(DEV))
    try:
        for shape, (R, N) in sorted(SHAPES.items()) + [("groups-37x129", (37, 129))]:
            batch = {k: v.to(DEV) for k, v in cases.neo_batch(cases.strided_rays(R), nv=nv).items()}
            far_g, _ = ops.intersect_sphere(batch["rays_o"], batch["rays_d"])
            for style in ("shared", "per-ray"):
                tv = _rows(style, R, N).to(DEV)
                for slot, _prefix in OUTSIDE:
                    res = {}
                    for width in (None,) + WIDTHS:
                        ctx.set_tp_quad(width)
                        res[width] = net.eval_mlp(slot, batch, tv, far=far_g).clone()
                    for width in (None, 4, 16):
                        assert torch.equal(res[width], res[0]), (shape, style, slot, width, float((res[width] - res[0]).abs().max()))
    finally:
        ctx.set_tp_quad(None)
