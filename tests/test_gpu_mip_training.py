"""GPU: Mip-NeRF 360's training call (mipnerf360/model.py:236-365 under LitMipNeRF360.training_step :436-470) on the operator chain
of training.mip_render_train: randomized proposal resampling (neo_mip_resample_u), IPE rows (neo_mip_encode), the MLPs on the
linear-layer operators, compositing with a native backward (neo_mip_composite_backward)."""
import pytest
import torch

import alongray_cases as A
import cases
import oracle
from conftest import max_abs, record_parity
from oracle import mip360
from neo360_amd import models, ops, synth, training

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = float(torch.finfo(torch.float32).eps)


def _net(counts=(16, 8)):
    net = models.MipNeRF360(num_prop_samples=counts[0], num_nerf_samples=counts[1]).to(DEV)
    net.load_state_dict(synth.mip360_state(0, weight_gain=0.25))
    return net


def _to(b):
    return {k: v.to(DEV) for k, v in b.items()}


def test_encode_rows_match_the_oracle():
    """neo_mip_encode = conical frustum -> Gaussian -> contraction -> lift -> integrated_pos_enc, reference feature order."""
    rays = cases.mip_rays(96)
    t = torch.sort(torch.rand(96, 33, generator=torch.Generator().manual_seed(5)) * 5.0 + 0.2, dim=-1).values
    basis = mip360.icosahedron_basis()
    got = training.mip_encode(rays["rays_o"].to(DEV), rays["rays_d"].to(DEV), rays["radii"].to(DEV), t.to(DEV), basis.to(DEV)).cpu()
    means, covs = mip360.conical_frustum_gaussians(t.double(), rays["rays_o"].double(), rays["rays_d"].double(), rays["radii"].double())
    z, c = mip360.contract(means, covs)
    lm, lv = mip360.lift_and_diagonalize(z, c, basis.double())
    want = mip360.integrated_pos_enc(lm, lv, 0, 12).reshape(-1, 504)
    # sin(2^11 x) of an fp32 x: the argument itself carries 2^11 ulp(x), so the bound is on the fp32 evaluation (same inputs)
    means32, covs32 = mip360.conical_frustum_gaussians(t, rays["rays_o"], rays["rays_d"], rays["radii"])
    z32, c32 = mip360.contract(means32, covs32)
    lm32, lv32 = mip360.lift_and_diagonalize(z32, c32, basis)
    want32 = mip360.integrated_pos_enc(lm32, lv32, 0, 12).reshape(-1, 504)
    noise = float((want32.double() - want).abs().max())
    assert float((got.double() - want).abs().max()) <= 2.0 * noise + 2e-6
    assert float((got.double() - want)[:, :63].abs().max()) <= 2e-5          # the low octaves are well conditioned


@pytest.mark.parametrize("dilate", [False, True])
def test_randomized_resampling_matches_the_oracle(dilate):
    """neo_mip_resample_u with one jitter per ray = helper.py:343-396 (single_jitter) on the same histogram."""
    R, n_prev, n = 128, 24, 32
    g = torch.Generator().manual_seed(11 + int(dilate))
    s_prev = torch.sort(torch.rand(R, n_prev + 1, generator=g), dim=-1).values
    s_prev[:, 0], s_prev[:, -1] = 0.0, 1.0
    w_prev = torch.rand(R, n_prev, generator=g) ** 3 + 1e-4
    w_prev = w_prev / w_prev.sum(-1, keepdim=True)
    u_max = EPS + (1 - EPS) / n
    max_jitter = (1 - u_max) / (n - 1) - EPS
    jitter = torch.rand(R, 1, generator=g) * max_jitter
    u = torch.linspace(0, 1 - u_max, n)
    sd, td = training.mip_resample_u(s_prev.to(DEV), w_prev.to(DEV), n, 0.2, 3.0, dilate, 0.01, 0.7, u.to(DEV), jitter.to(DEV))
    t, w = s_prev, w_prev
    if dilate:
        t, w = mip360.max_dilate_weights(t, w, 0.01, (0.0, 1.0))
        t, w = t[..., 1:-1], w[..., 1:-1]
    logits = torch.where(t[..., 1:] > t[..., :-1], 0.7 * torch.log(w), torch.full_like(w, -torch.inf))
    want = mip360.sample_intervals(t, logits, n, (0.0, 1.0), jitter)
    assert max_abs(sd.cpu(), want) <= 2e-5          # dilated histograms: 73 edges, a cdf step of 1e-7 moves a centre by up to 1e-5
    # and the deterministic table through the same entry point is neo_mip_resample bit for bit
    pad = 1 / (2 * n)
    a = training.mip_resample_u(s_prev.to(DEV), w_prev.to(DEV), n, 0.2, 3.0, dilate, 0.01, 0.7, torch.linspace(pad, 1 - pad - EPS, n).to(DEV))
    b = ops.mip_resample(s_prev.to(DEV), w_prev.to(DEV), n, 0.2, 3.0, dilate, 0.01, 0.7)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_composite_backward_matches_autograd():
    R, n = 200, 40
    g = torch.Generator().manual_seed(2)
    rgb = torch.rand(R, n, 3, generator=g)
    dens = torch.rand(R, n, generator=g) * 4.0
    dens[: R // 4] *= 0.02                              # thin rays: the background term is active
    t = torch.sort(torch.rand(R, n + 1, generator=g) * 4 + 0.2, dim=-1).values
    d = torch.randn(R, 3, generator=g)
    uw, uc = torch.randn(R, n, generator=g), torch.randn(R, 3, generator=g)
    with torch.enable_grad():
        a, b = rgb.to(DEV).requires_grad_(True), dens.to(DEV).requires_grad_(True)
        w, c = training.mip_composite(a, b, t.to(DEV), d.to(DEV), 1.0)
        got = torch.autograd.grad((w * uw.to(DEV)).sum() + (c * uc.to(DEV)).sum(), [a, b])
        a64, b64 = rgb.double().requires_grad_(True), dens.double().requires_grad_(True)
        w64 = mip360.alpha_weights(b64, t.double(), d.double())
        c64 = (w64[..., None] * a64).sum(-2) + torch.clip(1 - w64.sum(-1, keepdim=True), min=0) * 1.0
        want = torch.autograd.grad((w64 * uw.double()).sum() + (c64 * uc.double()).sum(), [a64, b64])
    # the bounds of the shared table (alongray_cases.mip_composite_checks): weights 2e-6, colour 5e-6, gradients entry by entry at
    # 2e-5 x max(1, largest |fp64 gradient|) - this compositing has no sentinel interval (its last one is opaque by construction)
    assert max_abs(w.detach().cpu().double(), w64.detach()) <= A.MIP_W and max_abs(c.detach().cpu().double(), c64.detach()) <= A.MIP_C
    ref = dict(weights=w64.detach(), rgb=c64.detach(), g_rgb=want[0], g_density=want[1])
    checks = A.mip_composite_checks(dict(weights=w.detach(), rgb=c.detach(), g_rgb=got[0], g_density=got[1]), ref, ref)
    A.assert_inside(checks, "mip composite backward")


def test_training_call_forward_equals_the_fused_kernels():
    net = _net((32, 16))
    rays = _to(cases.mip_rays(160))
    fused = net(rays, 0.6, False, False, 0.2, 3.0)
    net.differentiable = True
    with torch.enable_grad():
        chain = net(rays, 0.6, False, True, 0.2, 3.0)
    assert chain[0][2]["rgb"].requires_grad
    for lvl in range(3):
        assert max_abs(chain[1][lvl]["sdist"], fused[1][lvl]["sdist"]) < 1e-4
        assert max_abs(chain[0][lvl]["rgb"].detach(), fused[0][lvl]["rgb"]) < 1e-4
        assert max_abs(chain[1][lvl]["weights"].detach(), fused[1][lvl]["weights"]) < 1e-4


def test_training_step_gradients_vs_fp64_autograd():
    """A training_step-shaped loss - rgb L2 on the final level + a term on every level's interval weights (what the interlevel /
    distortion losses read) - on 96 randomized rays: gradients of all 44 parameter tensors against fp64 autograd of
    oracle.mip360.render at the library's sample positions AND encodings (profiles/r05_mip_train_gradients.log: on its own fp32
    encodings the reference's fp32 arithmetic misses the fp64 gradients of the 8 x 1024 trunk by 2e-3 - sin(2^k x) moves units
    across their ReLU kink - so the encodings are pinned by test_encode_rows_match_the_oracle and fed to both sides here).
    The library may miss the fp64 gradients by no more than 1.5 x what the reference's own fp32 arithmetic misses them by (+ 2e-5).
    One exception is structural: a unit whose pre-activation lies within fp32 rounding of zero takes the other derivative in a
    different summation order (the same log shows one such unit in layer 1 of the second proposal MLP: layers 0-1 off by 1e-3,
    everything above exact); such a flip may touch the trunk layers of ONE MLP, from some layer downwards, by <= 5e-3 in relative L2 (the unit's
    own weight row moves more: <= 3e-2 of the largest entry)."""
    R, counts = 96, (16, 8)
    net = _net(counts)
    sd = synth.mip360_state(0, weight_gain=0.25)
    rays_c = cases.mip_rays(R)
    rays = _to(rays_c)
    target = synth.uniform(93, "mip_target", (R, 3), 0.0, 1.0)
    level_n = (counts[0], counts[0], counts[1])
    probes = [synth.uniform(94 + l, "mip_probe", (R, n), 0.0, 1.0) for l, n in enumerate(level_n)]
    names = sorted(k for k in sd if not k.endswith("pos_basis_t"))
    with torch.enable_grad():
        for p in net.parameters():
            p.requires_grad_(True)
        rend, hist = training.mip_render_train(net, rays, 0.5, True, 0.2, 3.0, seed=13)
        loss_g = ((rend[2]["rgb"] - target.to(DEV)) ** 2).mean() + 0.05 * sum((h["weights"] * p.to(DEV)).sum(-1).mean() for h, p in zip(hist, probes))
        params = dict(net.named_parameters())
        g_g = torch.autograd.grad(loss_g, [params[k] for k in names])
        sdists = [h["sdist"].detach().cpu() for h in hist]
        x0s = []
        for sdv, n in zip(sdists, level_n):
            td = 1 / (sdv * (1 / 3.0) + (1 - sdv) * (1 / 0.2))
            x0s.append(training.mip_encode(rays["rays_o"], rays["rays_d"], rays["radii"], td.to(DEV), net.mlps[0].pos_basis_t).cpu().reshape(R, n, 504))

        def oracle_grads(dtype):
            cv = lambda v: v.to(dtype) if torch.is_floating_point(v) else v
            pp = {k: (cv(v).clone().requires_grad_(True) if k in names else cv(v)) for k, v in sd.items()}
            r2, h2 = mip360.render(pp, {k: cv(v) for k, v in rays_c.items()}, 0.5, 0.2, 3.0, num_prop_samples=counts[0],
                                   num_nerf_samples=counts[1], sdist_given=[cv(x) for x in sdists],
                                   basis=cv(mip360.icosahedron_basis()), x0_given=[cv(x) for x in x0s])
            loss = ((r2[2]["rgb"] - cv(target)) ** 2).mean() + 0.05 * sum((h["weights"] * cv(p)).sum(-1).mean() for h, p in zip(h2, probes))
            return float(loss.detach()), torch.autograd.grad(loss, [pp[k] for k in names])

        loss_c, g_c = oracle_grads(torch.float64)
        _, g_r = oracle_grads(torch.float32)
    assert abs(float(loss_g) - loss_c) < 2e-5 * max(1.0, abs(loss_c))
    rel = lambda x, ref: (float(x.abs().max()) / (float(ref.abs().max()) + 1e-15), float(x.norm()) / (float(ref.norm()) + 1e-30))
    worst, flipped = 0.0, []
    for nm, a, b, r in zip(names, g_g, g_c, g_r):
        a = a.detach().cpu().double()
        lib, ref = rel(a - b, b), rel(r.double() - b, b)
        if lib[0] <= 1.5 * ref[0] + 2e-5 and lib[1] <= 1.5 * ref[1] + 2e-5:
            worst = max(worst, lib[1])
        else:
            flipped.append((nm, lib, ref))
    if flipped:
        mlps = {nm.split(".pts_linear.")[0] for nm, _, _ in flipped}
        layers = sorted({int(nm.split(".pts_linear.")[1].split(".")[0]) for nm, _, _ in flipped if ".pts_linear." in nm})
        assert len(mlps) == 1 and all(".pts_linear." in nm and lib[1] <= 5e-3 and lib[0] <= 3e-2 for nm, lib, _ in flipped), flipped
        assert layers == list(range(layers[-1] + 1)), flipped             # from one layer downwards
    record_parity("train_mip360_module_call", max_rel_l2_grad_err_vs_fp64=worst, rays=R, loss_abs_err=abs(float(loss_g) - loss_c),
                  tensors_below_a_flipped_unit=[nm for nm, _, _ in flipped])


@pytest.mark.parametrize("lvl", [0, 2])
def test_fused_chain_equals_the_per_layer_operators(lvl):
    """neo_mip_mlp_train_forward / _backward (one native chain each way, round 6: trunk, skip layer, heads, softplus / sigmoid inside
    the library) against mip_mlp (one operator per layer + torch glue) on a proposal MLP (4 x 256, no colour) and the NeRF MLP
    (8 x 1024): the same exact-fp32 GEMMs, so outputs and every parameter gradient agree to rounding of the summation order."""
    R, n = 72, 24
    net = _net()
    mlp = net.mlps[lvl]
    g = torch.Generator(device=DEV).manual_seed(3 + lvl)
    x0 = torch.randn(R * n, 504, device=DEV, generator=g).clamp_(-1, 1)
    d_enc = torch.randn(R, 27, device=DEV, generator=g)
    up_d, up_c = torch.randn(R, n, device=DEV, generator=g), torch.randn(R, n, 3, device=DEV, generator=g)
    layers = mlp.ordered_layers()
    params = [l.weight for l in layers] + [l.bias for l in layers]
    res = []
    with torch.enable_grad():
        for p in params:
            p.requires_grad_(True)
        for fn in (training.mip_mlp_fused, training.mip_mlp):
            dens, rgb = fn(mlp, x0, d_enc, n)
            loss = (dens * up_d).sum() + (rgb * up_c).sum() if not mlp.disable_rgb else (dens * up_d).sum()
            res.append((dens.detach(), rgb.detach(), torch.autograd.grad(loss, params)))
    (d_a, c_a, g_a), (d_b, c_b, g_b) = res
    assert d_a.shape == (R, n) and c_a.shape == (R, n, 3)
    assert max_abs(d_a, d_b) <= 3e-6 * max(1.0, float(d_b.abs().max())) and max_abs(c_a, c_b) <= 3e-6
    for i, (a, b) in enumerate(zip(g_a, g_b)):
        assert float((a - b).abs().max()) <= 2e-5 * max(float(b.abs().max()), 1e-6), (i, float((a - b).abs().max()), float(b.abs().max()))
