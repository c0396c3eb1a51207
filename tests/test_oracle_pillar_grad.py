"""CPU: fp64 autograd of oracle.pillar.floorplans against the gradients the reference's own GridEncoder back-propagates
(g11_pillar_grad, tests/golden/make_golden_pillar_grad.py): ties the oracle's pillar-stage gradients - the yardstick of
tests/test_gpu_encoder_training.py - to the reference."""
import torch

import cases
import oracle
from neo360_amd import synth

SEED_G = 11


def _layers():
    layers = ["depth_fc.common_branch.0", "depth_fc.common_branch.2", "depth_fc.depth_encoder"]
    for ax in ("xz", "yz", "xy"):
        layers += ["pillar_aggregator_%s.0" % ax, "pillar_aggregator_%s.2" % ax]
    return layers


def _rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm()) / (float(b.norm()) + 1e-30)


def test_oracle_pillar_gradients_vs_reference_fixture(golden):
    g = golden("g11_pillar_grad")
    torch.set_num_threads(8)
    grid = (12, 10, 8)
    G0, G1, G2 = grid
    nv = cases.NV
    params = {k: v.double().requires_grad_(True) for k, v in synth.pillar_state(0).items()}
    latent = cases.small_scene()["latent"].double().requires_grad_(True)
    poses, focal, centre = synth.source_views(nv, *cases.IMG_WH)
    with torch.enable_grad():
        fps = oracle.pillar.floorplans(params, latent, cases.small_scene()["image_wh"], poses.double(), focal.double(),
                                       centre.double(), grid)
        shapes = {"yz": (nv, G1, G2, 512), "xz": (nv, G0, G2, 512), "xy": (nv, G0, G1, 512)}
        cot = [synth.normal(SEED_G, "pillar_grad_" + k, shapes[k], 1.0).double() for k in ("yz", "xz", "xy")]
        loss = sum((a * c).sum() for a, c in zip(fps, cot))
        names = _layers()
        ins = [params[n + ".weight"] for n in names] + [params[n + ".bias"] for n in names] + [latent]
        grads = torch.autograd.grad(loss, ins)
    # the fixture is the reference's fp32 arithmetic: a few 1e-6 relative from fp64 (measured <= 2e-5)
    for n, gw in zip(names, grads[:9]):
        key = (n + ".weight").replace(".", "_")
        assert _rel_l2(gw[::32], g["rows_" + key]) < 1e-4, n
        assert _rel_l2(gw.sum(1), g["sum_" + key]) < 1e-4, n
        assert _rel_l2((gw ** 2).sum(1), g["sq_" + key]) < 1e-4, n
    for n, gb in zip(names, grads[9:18]):
        want = g[(n + ".bias").replace(".", "_")]
        if n.endswith(".2") and "aggregator" in n:
            # a scorer head's bias shifts every score of a pillar alike and the softmax ignores it: its gradient is zero, and
            # the reference's fp32 arithmetic leaves ~5e-6 of rounding there
            assert float(gb.abs().max()) < 1e-9 and abs(float(want[0])) < 1e-4, (n, float(gb[0]), float(want[0]))
        else:
            assert _rel_l2(gb, want) < 1e-4, n
    assert _rel_l2(grads[18].reshape(-1)[::389], g["latent_strided"]) < 1e-4
