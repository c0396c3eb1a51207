"""CPU: the oracle against the reference itself - the reference's outputs of exactly these calls (same inputs, same seeds) are
the committed fixture tests/golden/g10_live.npz, produced by tests/golden/make_golden.py (`g10`) with the reference imported under
the import stubs of tests/golden/_ref_loader.py."""
import torch

import cases
import oracle
from conftest import max_abs
from neo360_amd import synth


def test_vanilla_forward_live(golden):
    g = golden("g10_live")
    state = synth.vanilla_state(0)
    rays = cases.strided_rays(64)
    got = oracle.vanilla.render(state, rays, 0.2, 3.0)
    assert max_abs(got[0][0], g["van_rgb0"]) < 1e-6 and max_abs(got[1][0], g["van_rgb1"]) < 5e-6
    assert max_abs(got[1][2], g["van_depth1"]) < 5e-5


def test_pixelnerf_mlp_stage_live(golden):
    """The PixelNeRF late-fusion MLP (vanilla_nerf/model_pixel.py:96-131) on synthetic encodings / latents."""
    g = golden("g10_live")
    for nv in (1, 3):
        sd = synth.pixelnerf_mlp_state(61 + nv, "")
        P = 40
        x = synth.uniform(63, "pix_x%d" % nv, (nv, P, 63), -1, 1)
        cond = synth.uniform(63, "pix_c%d" % nv, (nv * P, 27), -1, 1)
        latent = synth.normal(63, "pix_l%d" % nv, (nv * P, 512), 0.3)
        rr, ss = oracle.mlp.pixelnerf_mlp(sd, "", x, cond, latent, nv)
        assert max_abs(rr, g["pixmlp_rgb_nv%d" % nv]) < 1e-6 and max_abs(ss, g["pixmlp_sigma_nv%d" % nv]) < 1e-6


def test_pixelnerf_forward_live(golden):
    g = golden("g10_live")
    scene = cases.small_scene()
    state = synth.pixelnerf_state(0)
    batch = cases.neo_batch(cases.strided_rays(48))
    got = oracle.pixelnerf.render(state, batch, scene, 0.2, 2.5)
    assert max_abs(got[0][0], g["pix_rgb0"]) < 1e-6
    assert max_abs(got[1][0], g["pix_rgb1"]) < 1e-5 and max_abs(got[1][2], g["pix_depth1"]) < 5e-5


def test_neo360_forward_live(golden):
    g = golden("g10_live")
    scene = cases.small_scene()
    state = synth.nerf_tp_state(0)
    batch = cases.neo_batch(cases.strided_rays(40))
    got = oracle.neo360.render(state, batch, scene, 24, 40)
    assert max_abs(got[0][0], g["neo_rgb0"]) < 5e-6 and max_abs(got[1][0], g["neo_rgb1"]) < 5e-6
    assert max_abs(got[1][5], g["neo_out5_1"]) < 5e-5 and max_abs(got[1][4], g["neo_out4_1"]) < 5e-6


def test_mip360_forward_live(golden):
    g = golden("g10_live")
    state = synth.mip360_state(0, weight_gain=0.5)
    rays = cases.mip_rays(24)
    from oracle import mip360
    got, ghist = mip360.render(state, rays, 1.0, 0.2, 3.0, num_prop_samples=32, num_nerf_samples=16)
    assert max_abs(got[-1]["rgb"], g["mip_rgb"]) < 5e-6
    assert max_abs(ghist[-1]["sdist"], g["mip_sdist"]) < 5e-6


def _reference_gradients(g, state):
    """The reference's autograd gradients of every linear layer, rebuilt from what crossed each MLP's boundary in its forward /
    backward (make_golden.py g10_live checks the rebuild against the reference's own result to 1e-5)."""
    out = {}
    for m in ("mlps.0", "mlps.1", "mlps.2"):
        tag = m.replace(".", "")
        out.update(cases.mip_mlp_param_grads(state, m + ".", g["rnd_x0_" + tag], g["rnd_dyd_" + tag], g.get("rnd_dir_" + tag),
                                             g.get("rnd_dyrgb_" + tag)))
    return out


def test_mip360_randomized_forward_and_gradients_live(golden):
    """The reference's randomized training forward (one jitter per ray and level, helper.py:358-365) and its autograd gradients
    against the oracle fed the SAME draws: torch.rand is consumed by the reference in level order, (B, 1) per level, so the oracle's
    `jitters` are reproduced from the same seed.  Pins the oracle hooks the GPU training tests rely on (`jitters`, `sdist_given`)."""
    g_ref = golden("g10_live")
    n_prop, n_nerf, B = 16, 8, 12
    state = synth.mip360_state(0, weight_gain=0.25)
    rays = cases.mip_rays(B)
    eps = float(torch.finfo(torch.float32).eps)
    names = bytes(g_ref["rnd_names"].numpy()).decode().split("\n")
    unused = [bool(u) for u in g_ref["rnd_unused"]]
    torch.manual_seed(5)
    jit = []
    for n in (n_prop, n_prop, n_nerf):
        u_max = eps + (1 - eps) / n
        jit.append(torch.rand(B, 1) * ((1 - u_max) / (n - 1) - eps))
    from oracle import mip360
    with torch.enable_grad():
        pp = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in state.items()}
        got, ghist = mip360.render(pp, rays, 0.5, 0.2, 3.0, num_prop_samples=n_prop, num_nerf_samples=n_nerf, jitters=jit)
        loss = (got[-1]["rgb"] ** 2).mean() + sum((h["weights"] ** 2).sum(-1).mean() for h in ghist)
        g = torch.autograd.grad(loss, [pp[k] for k in names], allow_unused=True)
    for lvl in range(3):
        assert max_abs(ghist[lvl]["sdist"], g_ref["rnd_sdist%d" % lvl]) < 5e-6, lvl
        assert max_abs(ghist[lvl]["weights"].detach(), g_ref["rnd_w%d" % lvl]) < 2e-5, lvl
    assert max_abs(got[-1]["rgb"].detach(), g_ref["rnd_rgb"]) < 5e-6
    grads_ref = _reference_gradients(g_ref, state)
    for k, a, none_ref in zip(names, g, unused):
        assert (a is None) == none_ref, k
        if a is not None:
            b = grads_ref[k]
            assert float((a - b).norm()) <= 2e-3 * float(b.norm()) + 1e-9, k       # fp32 autograd of two op orders (ReLU-kink flips: see profiles/r05_mip_train_gradients.log)
    # evaluating at GIVEN interval endpoints reproduces the same forward
    again, _ = mip360.render(state, rays, 0.5, 0.2, 3.0, num_prop_samples=n_prop, num_nerf_samples=n_nerf,
                             sdist_given=[g_ref["rnd_sdist%d" % lvl] for lvl in range(3)])
    assert max_abs(again[-1]["rgb"], g_ref["rnd_rgb"]) < 5e-6
