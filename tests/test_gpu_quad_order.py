"""GPU: the quad order of the pre-projected split evaluators (csrc/point_order.h:quad_point, neo_ctx_set_tp_quad) is pure
scheduling - every tensor a call returns is bitwise the ray-major one.

In quad order a 64-point tile holds 64 / G samples of G consecutive launch-order rays (G = 4: a quad; 16: the widest
group) instead of 64 samples of one ray; which points share a tile must not show in any result.  Forced on (1 = quads of four, and
16 rays per group) against forced off (0) through the context setter, in one process:

* calls: the default two-level evaluation call (both levels, all six tensors each: the eight outputs of the end-to-end contract
  among them), the `fine_only` frame call (density-only coarse launches), and the per-point stage entry `eval_mlp` of all four
  slots at the render's own sample positions;
* shapes: R in {1, 3, 4, 5, 67, 131} at 128 + 256 samples - no quad at all, a partial last quad, a tile straddling two quads
  (4 x 129 = 516 = 8 tiles + 4 points; 16 x 129 = 2064 = 32 tiles + 16 points) and P no multiple of 64; 67 and 131 rays are four /
  eight groups of 16 and three rays in ray-major order; reference chunk 6 and 64, so that a chunk boundary (quirk Q1: the
  direction a point carries is taken from another ray of its chunk) falls inside a quad;
* with and without the pixel-grid hint (8 pixels wide: 67 / 131 rays end in a ragged band; first_ray = 5 makes both ends ragged);
* 1 and 3 source views; pre-projection modes 1, 2 and 3, so that k_tp_mlp_hp<3>, <4> and k_tp_mlp_hpp<3>, <4> all run; f16x3 only;
* a culled call (compact background launches never take the order) with the mode forced on is bitwise the call with it off, and
  the library's default choice is bitwise both.
"""
import pytest
import torch

import cases
from neo360_amd import models, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
RAYS = (1, 3, 4, 5, 67, 131)
CHUNKS = (6, 64)
GRIDS = (None, (8, 0), (8, 5))


def _net(nv, preproject, fg_bias=0.0):
    net = models.NeRF_TP(num_coarse_samples=128, num_fine_samples=256, num_src_views=nv).to(DEV)
    st = synth.nerf_tp_state(0)
    for k in ("fg_coarse_mlp.density_layer.bias", "fg_fine_mlp.density_layer.bias"):
        st[k] = st[k] + fg_bias
    net.load_state_dict(st)
    sc = cases.small_scene(nv=nv)
    net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV),
                  sc["image_wh"], preproject=preproject)
    assert (net.precision or net.default_precision) == "f16x3"
    return net


def _batch(n, nv):
    return {k: v.to(DEV) for k, v in cases.neo_batch(cases.strided_rays(n), nv=nv).items()}


def _calls(net, batch, chunk, grid):
    """Every tensor of the three kinds of call, cloned, in a fixed order."""
    out = []
    net.ray_grid = grid
    try:
        full = net(batch, False, False, 0.0, 0.0, out_depth=True, chunk=chunk)
        net.check_flags()
        out += [("full level %d [%d]" % (lv, i), t.clone()) for lv in range(2) for i, t in enumerate(full[lv])]
        fine = net(batch, False, False, 0.0, 0.0, out_depth=True, chunk=chunk, fine_only=True)
        net.check_flags()
        assert fine[0] is None
        out += [("fine_only [%d]" % i, t.clone()) for i, t in enumerate(fine[1])]
    finally:
        net.ray_grid = None
    return out


def _stage(net, batch, chunk, pos, far):
    out = []
    for slot in range(4):
        fg_t, bg_s = pos[slot & 1]
        out.append(("eval_mlp slot %d" % slot, net.eval_mlp(slot, batch, fg_t if slot < 2 else bg_s, far=far, chunk=chunk).clone()))
    return out


def _assert_same(on, off, label):
    assert len(on) == len(off) and len(on) > 0
    for (ka, a), (kb, b) in zip(on, off):
        assert ka == kb and a.shape == b.shape, (label, ka, kb)
        assert torch.equal(a, b), (label, ka, "quad order changed a result", float((a - b).abs().max()))


@pytest.mark.parametrize("preproject", [1, 2, 3], ids=["pre1-hp", "pre2-hpp", "pre3-mix"])
@pytest.mark.parametrize("nv", [1, 3], ids=["1view", "3views"])
def test_quad_order_on_and_off_are_bitwise_equal(nv, preproject):
    net = _net(nv, preproject)
    ctx = net._context(torch.device(DEV))
    try:
        for R in RAYS:
            batch = _batch(R, nv)
            far, _ = ops.intersect_sphere(batch["rays_o"], batch["rays_d"])
            for chunk in CHUNKS:
                ctx.set_tp_quad(0)
                pos = [(a.clone(), b.clone()) for a, b in net.sample_positions(batch, chunk=chunk)]
                res = {}
                for mode in (0, 1, 16):
                    ctx.set_tp_quad(mode)
                    res[mode] = _stage(net, batch, chunk, pos, far)
                    for grid in GRIDS:
                        res[mode] += [("%s grid %s" % (k, grid), t) for k, t in _calls(net, batch, chunk, grid)]
                _assert_same(res[1], res[0], (R, chunk, "quads"))
                _assert_same(res[16], res[0], (R, chunk, "groups of 16"))
                assert all(bool(torch.isfinite(t).all()) for _, t in res[0])
        assert ctx.poll_flags() == 0
    finally:
        ctx.set_tp_quad(None)


def test_library_default_is_bitwise_both():
    net = _net(3, 3)
    ctx = net._context(torch.device(DEV))
    batch = _batch(131, 3)
    try:
        res = {}
        for mode in (None, 0, 1, 8, 16):
            ctx.set_tp_quad(mode)
            res[mode] = _calls(net, batch, 64, (8, 0))
    finally:
        ctx.set_tp_quad(None)
    _assert_same(res[None], res[0], "default vs off")
    for mode in (1, 8, 16):
        _assert_same(res[mode], res[0], "%d vs off" % mode)


@pytest.mark.parametrize("preproject", [1, 3], ids=["pre1-hp", "pre3-mix"])
def test_culled_call_with_the_mode_forced_on_is_bitwise_the_call_without(preproject):
    """cull_background set: the background launches are COMPACT (rows are map entries, the ray count lives on the device) and
    never take the order; the foreground launches do.  Foreground density bias + 4 makes a mixed frame at eps = 1e-2
    (tests/test_gpu_cull_background.py)."""
    net = _net(3, preproject, fg_bias=4.0)
    ctx = net._context(torch.device(DEV))
    batch = _batch(70, 3)
    net.cull_background = 1e-2
    try:
        res, survivors = {}, {}
        for mode in (0, 1, 16):
            ctx.set_tp_quad(mode)
            res[mode] = _calls(net, batch, 6, (8, 0))
            survivors[mode] = int(net.last_cull_survivors)
    finally:
        net.cull_background = None
        ctx.set_tp_quad(None)
    assert 0 < survivors[0] < 70, "the case needs a mixed frame, %d of 70 rays survive" % survivors[0]
    assert survivors[1] == survivors[0] == survivors[16]
    _assert_same(res[1], res[0], "culled, quads")
    _assert_same(res[16], res[0], "culled, groups of 16")
