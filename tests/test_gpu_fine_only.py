"""GPU: `NeRF_TP.forward(..., out_depth=True, fine_only=True)` - the frame path's call - against the default call.

With `fine_only=True` the library gets a NULL level 0: the coarse launches of both regions run the DENSITY-ONLY
instantiations of the pre-projected split evaluators (k_tp_mlp_hp / k_tp_mlp_hpp: no direction staging, no view layers, no rgb
head, no per-ray direction sums) and the coarse composites write weights only.  The contract:

* `[1]` of the call is bitwise `[1]` of the default call, all six tensors.  Every fine sample position is a function of every
  coarse sigma of its ray (the resampler's cdf), so bitwise-equal fine rgb / depth IS the check that the density-only kernels
  produce the full kernels' sigma bits;
* `[0]` is None, and the flags word is clean after both calls.

Shapes: 70 rays x 129 / 385 samples (129 is no multiple of the 64-point tile: tiles straddle rays, the last tile is partial);
70 rays x 9 / 25 samples (several rays per tile); 1 and 3 source views; pre-projection modes 1 (k_tp_mlp_hp on all four slots),
2 (k_tp_mlp_hpp on all four) and 3 (the default mix); the ray-grid hint (patch tile order); the culled call (compact
density-only background launch); and the evaluators that ignore the hint (exact fp32, raw-latent split).
"""
import pytest
import torch

import cases
from neo360_amd import models, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("rgb", "fg_rgb", "bg_rgb", "fg_acc", "bg_lambda", "depth")


def _net(nv=3, preproject=3, n_coarse=128, n_fine=256, precision=None, fg_bias=0.0):
    net = models.NeRF_TP(num_coarse_samples=n_coarse, num_fine_samples=n_fine, num_src_views=nv).to(DEV)
    st = synth.nerf_tp_state(0)
    for k in ("fg_coarse_mlp.density_layer.bias", "fg_fine_mlp.density_layer.bias"):
        st[k] = st[k] + fg_bias
    net.load_state_dict(st)
    sc = cases.small_scene(nv=nv)
    net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV),
                  sc["image_wh"], preproject=preproject)
    if precision is not None:
        net.precision = precision
    return net


def _batch(n, nv=3):
    return {k: v.to(DEV) for k, v in cases.neo_batch(cases.strided_rays(n), nv=nv).items()}


def _both(net, batch, chunk=None):
    full = net(batch, False, False, 0.0, 0.0, out_depth=True, chunk=chunk)
    net.check_flags()
    full = [[t.clone() for t in lv] for lv in full]
    fine = net(batch, False, False, 0.0, 0.0, out_depth=True, chunk=chunk, fine_only=True)
    net.check_flags()
    assert net._context(torch.device(DEV)).poll_flags() == 0
    return full, fine


def _assert_fine_equal(full, fine):
    assert len(fine) == 2 and fine[0] is None
    assert len(fine[1]) == 6
    for k, a, b in zip(NAMES, fine[1], full[1]):
        assert a.shape == b.shape, k
        assert torch.equal(a, b), ("level 1 of the fine-only call must be bitwise the default call's", k,
                                   float((a - b).abs().max()))


SHAPES = [(128, 256), (8, 16)]


@pytest.mark.parametrize("preproject", [1, 2, 3], ids=["pre1-hp", "pre2-hpp", "pre3-mix"])
@pytest.mark.parametrize("nv", [1, 3], ids=["1view", "3views"])
@pytest.mark.parametrize("n_coarse,n_fine", SHAPES, ids=["128+256", "8+16"])
def test_fine_only_level1_is_bitwise_the_default_call(n_coarse, n_fine, nv, preproject):
    net = _net(nv=nv, preproject=preproject, n_coarse=n_coarse, n_fine=n_fine)
    full, fine = _both(net, _batch(70, nv))
    _assert_fine_equal(full, fine)


def test_fine_only_under_the_ray_grid_hint():
    """128 rays as a 16-pixel-wide grid: the evaluators walk the rays in patches (2 x 2 inside, 8 x 8 outside the sphere)."""
    net = _net()
    batch = _batch(128)
    plain, _ = _both(net, batch)
    net.ray_grid = (16, 0)
    try:
        full, fine = _both(net, batch)
    finally:
        net.ray_grid = None
    _assert_fine_equal(full, fine)
    _assert_fine_equal(plain, fine)          # and the hint itself stays bitwise-neutral


@pytest.mark.parametrize("preproject", [1, 3], ids=["pre1-hp", "pre3-mix"])
def test_fine_only_culled_call(preproject):
    """cull_background set: the coarse background launch is the COMPACT density-only instantiation.  Foreground density bias + 4
    makes a mixed frame at eps = 1e-2 (tests/test_gpu_cull_background.py)."""
    net = _net(preproject=preproject, fg_bias=4.0)
    batch = _batch(70)
    net.cull_background = 1e-2
    try:
        full = net(batch, False, False, 0.0, 0.0, out_depth=True)
        net.check_flags()
        full = [[t.clone() for t in lv] for lv in full]
        n_full = int(net.last_cull_survivors)
        fine = net(batch, False, False, 0.0, 0.0, out_depth=True, fine_only=True)
        net.check_flags()
        n_fine = int(net.last_cull_survivors)
    finally:
        net.cull_background = None
    assert 0 < n_full < 70, "the case needs a mixed frame, %d of 70 rays survive" % n_full
    assert n_fine == n_full
    _assert_fine_equal(full, fine)


@pytest.mark.parametrize("precision,preproject", [("f32", 3), ("f16x3", False)], ids=["exact-f32", "raw-latent-split"])
def test_fine_only_on_evaluators_that_ignore_the_hint(precision, preproject):
    net = _net(preproject=preproject, precision=precision)
    full, fine = _both(net, _batch(70))
    _assert_fine_equal(full, fine)


def test_default_call_still_returns_both_levels():
    net = _net(n_coarse=8, n_fine=16)
    res = net(_batch(70), False, False, 0.0, 0.0, out_depth=True)
    assert len(res) == 2 and all(len(lv) == 6 and all(t is not None for t in lv) for lv in res)
    assert all(bool(torch.isfinite(t).all()) for lv in res for t in lv)
    net.check_flags()
