"""Generates tests/golden/g11_pillar_grad.npz: gradients of the REFERENCE's GridEncoder pillar stage (ResNet stubbed, as
make_golden.py:g9_pillar; grid (12, 10, 8), 3 views, cases.small_scene() latent, synth.pillar_state(0)) under seeded
cotangents on the three floor-plans.  The cotangents are not stored: synth's hash generator regenerates them
(tests/test_gpu_encoder_training.py:_cotangents, tests/test_oracle_pillar_grad.py).  Build-container only.

Stored (fp32; the file stays near 0.2 MB): every 32nd row of each weight gradient (every 8th would be 0.8 MB), per-row
sums and sums of squares of each weight gradient (fp64), every bias gradient, and every 389th entry of the flattened
latent gradient.

    python tests/golden/make_golden_pillar_grad.py
"""
import contextlib
import io
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
from make_golden import cases, ref, save, synth  # noqa: E402

SEED_G = 11
GRID = mg.PILLAR_GRID


def cotangents(grid, nv=cases.NV):
    G0, G1, G2 = grid
    shapes = {"yz": (nv, G1, G2, 512), "xz": (nv, G0, G2, 512), "xy": (nv, G0, G1, 512)}
    return {k: synth.normal(SEED_G, "pillar_grad_" + k, shapes[k], 1.0) for k in ("yz", "xz", "xy")}


def layer_names():
    layers = ["depth_fc.common_branch.0", "depth_fc.common_branch.2", "depth_fc.depth_encoder"]
    for ax in ("xz", "yz", "xy"):
        layers += ["pillar_aggregator_%s.0" % ax, "pillar_aggregator_%s.2" % ax]
    return layers


def g11_pillar_grad():
    torch.set_grad_enabled(True)
    ENC = ref.load("models.neo360.encoder_tp_fusion_conv")
    with contextlib.redirect_stdout(io.StringIO()):
        enc = ENC.GridEncoder(grid_size=list(GRID))
    missing = enc.load_state_dict(synth.pillar_state(0), strict=False)
    assert not missing.unexpected_keys, missing
    enc.eval()
    latent = cases.small_scene()["latent"].clone().requires_grad_(True)
    Hf, Wf = latent.shape[-2:]
    ls = torch.tensor([float(Wf), float(Hf)])
    sp = enc.spatial_encoder
    sp.forward = lambda images: None
    sp.latent = latent
    sp.latent_scaling = ls / (ls - 1) * 2.0
    captured = {}
    for ax in ("yz", "xz", "xy"):
        getattr(enc, "floorplan_convnet_" + ax).register_forward_pre_hook(
            lambda mod, inp, ax=ax: captured.__setitem__(ax, inp[0]))
    poses, focal, centre = synth.source_views(cases.NV, *cases.IMG_WH)
    images = torch.zeros(cases.NV, 3, cases.IMG_WH[1], cases.IMG_WH[0])
    real_tensor = torch.tensor
    torch.tensor = lambda *a, **k: real_tensor(*a, **{kk: vv for kk, vv in k.items() if kk != "device"})   # :465 hard-codes "cuda"
    try:
        enc(images, poses, focal, centre)
    finally:
        torch.tensor = real_tensor
    cot = cotangents(GRID)
    # the conv nets receive NCHW permutes of the channels-last floor-plans (:580-592)
    loss = sum((captured[ax].permute(0, 2, 3, 1) * cot[ax]).sum() for ax in ("yz", "xz", "xy"))
    params = dict(enc.named_parameters())
    names = layer_names()
    ins = [params[n + ".weight"] for n in names] + [params[n + ".bias"] for n in names] + [latent]
    grads = torch.autograd.grad(loss, ins)
    out = {}
    for n, g in zip(names, grads[:9]):
        key = (n + ".weight").replace(".", "_")
        g = g.double()
        out["rows_" + key] = g[::32].float()
        out["sum_" + key] = g.sum(1)
        out["sq_" + key] = (g ** 2).sum(1)
    for n, g in zip(names, grads[9:18]):
        out[(n + ".bias").replace(".", "_")] = g.float()
    out["latent_strided"] = grads[18].float().reshape(-1)[::389]
    save("g11_pillar_grad", **out)


if __name__ == "__main__":
    if not ref.reference_available():
        sys.exit("reference tree not found at %s" % ref.REFERENCE_ROOT)
    g11_pillar_grad()
