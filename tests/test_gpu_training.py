"""GPU: training-side operators through the C ABI against the oracle: counter-based uniforms
(bit-exact), stratified / randomized samplers, compositing backward, lookups forward + backward, distortion loss,
and NeRF_TP's training-mode forward (out_depth=False) against the reference-generated fixture g8_training."""
import pytest
import torch

import alongray_cases as A
import cases
import oracle
from conftest import max_abs
from neo360_amd import models, ops, synth, training
from oracle import training as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, NR, NC, NF = 1234, 64, 16, 24


def test_uniforms_bit_exact():
    for seed, stream, rows, cols in ((SEED, 0, 64, 17), (2 ** 40 + 12345, 3, 300, 129), (1, 9, 1, 1)):
        got = training.rand_uniform(seed, stream, rows, cols).cpu()
        assert torch.equal(got, T.philox_uniform(seed, stream, rows, cols))


def test_samplers_vs_reference_fixture(golden):
    g = golden("g8_training")
    rays = {k: v.to(DEV) for k, v in cases.strided_rays(NR).items()}
    far, _ = ops.intersect_sphere(rays["rays_o"], rays["rays_d"])
    u0, u1 = training.rand_uniform(SEED, 0, NR, NC + 1), training.rand_uniform(SEED, 1, NR, NC + 1)
    fg, bg = training.sample_level0(far, NC, u0, u1)
    assert max_abs(fg, g["strat_fg"]) < 5e-7 and max_abs(bg, g["strat_bg"]) < 2e-7     # fg carries the fp32 far of each ray
    fg_d, bg_d = training.sample_level0(far, NC)                      # randomized=False
    far_c, _ = oracle.rays.sphere_exit_depth(rays["rays_o"].cpu(), rays["rays_d"].cpu())
    want, _ = oracle.sampling.neo_fg_level0(rays["rays_o"].cpu(), rays["rays_d"].cpu(), NC, torch.full_like(far_c, 1e-4), far_c)
    assert max_abs(fg_d, want) < 5e-7                                  # one ulp of t near far (far itself is 1 ulp apart on the two sides)
    # randomized pdf sampling: the new samples are a permutation-free comparison after sorting (the op returns the merged set)
    pc = cases.pdf_cases()
    mids, w = pc["asc"]
    up = training.rand_uniform(SEED, 7, mids.shape[0], 48)
    # reconstruct a t_prev whose midpoints are `mids`: use the oracle path on the op's own convention instead
    t_prev = torch.sort(torch.rand(mids.shape[0], 33, generator=torch.Generator().manual_seed(1)), dim=-1).values
    wts = torch.rand(mids.shape[0], 33, generator=torch.Generator().manual_seed(2))
    for desc in (False, True):
        tp = torch.flip(t_prev, dims=[-1]) if desc else t_prev
        got = training.resample_u(tp.to(DEV), wts.to(DEV), up, descending=desc).cpu()
        want = T.resample_randomized(tp, wts, up.cpu(), descending=desc)
        assert got.shape == want.shape
        assert float((got - want).abs().median()) < 1e-6 and float((got - want).abs().quantile(0.99)) < 1e-4


@pytest.mark.parametrize("mode,white", [(0, False), (0, True), (1, False), (1, True), (2, False), (2, True)])
def test_composite_backward_matches_autograd(mode, white):
    """cases.composite_case() (64 rays x 129 samples) through training.composite against the fp64 oracle under autograd.  The
    density gradient is bounded ENTRY BY ENTRY (alongray_cases.sigma_grad_bounds): ray 0 is empty, so in modes 0 and 2 its last
    sample - the 1e10 sentinel interval - has a gradient of 1e10 G, and one bound scaled by the tensor's largest entry (what this
    test asserted before) let every other entry be wrong by 1e5."""
    inp, ref64, ref32 = A.composite_case(mode, 129, white, 64, True, None, True)
    rgb, sigma, t, dirs, far, up = (inp[k] for k in ("rgb", "sigma", "t", "dirs", "far", "up"))
    with torch.enable_grad():
        rg, sg = rgb.clone().to(DEV).requires_grad_(True), sigma.clone().to(DEV).requires_grad_(True)
        d_g = dirs.to(DEV) if mode != 2 else None
        o_rgb, o_acc, o_w, o_lam, o_depth = training.composite(mode, rg, sg, t.to(DEV), d_g, far.to(DEV) if mode == 1 else None, white)
        loss_g = ((o_rgb * up["rgb"].to(DEV)).sum() + (o_acc * up["acc"].to(DEV)).sum() + (o_w * up["weights"].to(DEV)).sum() +
                  (o_depth * up["depth"].to(DEV)).sum() + ((o_lam * up["lam"].to(DEV)).sum() if mode == 1 else 0.0))
        g_rgb_g, g_sig_g = torch.autograd.grad(loss_g, [rg, sg])
    assert max_abs(o_rgb, ref64["rgb"]) < 2e-6 and max_abs(o_w, ref64["weights"]) < 2e-6
    assert max_abs(g_rgb_g, ref64["g_rgb"]) < 2e-6 * max(1.0, float(ref64["g_rgb"].abs().max()))
    max_abs(g_sig_g[..., 0], ref64["g_sigma"])                                  # into the parity report
    checks = A.composite_checks(dict(g_rgb=g_rgb_g.cpu(), g_sigma=g_sig_g[..., 0].cpu()), mode, ref64, ref32)
    A.assert_inside(checks, ("composite backward", mode, white))


def test_distloss_forward_backward():
    gen = torch.Generator().manual_seed(5)
    w = torch.rand(200, 385, generator=gen)
    w = w / w.sum(-1, keepdim=True) * torch.rand(200, 1, generator=gen)
    m = torch.sort(torch.rand(200, 385, generator=gen), dim=-1).values
    with torch.enable_grad():
        wc = w.double().requires_grad_(True)
        lc = T.eff_distloss(wc, m.double(), 1.0 / 385)
        (gc,) = torch.autograd.grad(lc * 3.0, wc)
        wg = w.to(DEV).requires_grad_(True)
        lg = training.eff_distloss(wg, m.to(DEV), 1.0 / 385)
        (gg,) = torch.autograd.grad(lg * 3.0, wg)
    assert abs(float(lg) - float(lc)) < 1e-6 * max(1.0, abs(float(lc)))
    assert max_abs(gg, gc) < 1e-6 * max(1.0, float(gc.abs().max()))


def test_gather_forward_and_backward():
    sc = cases.small_scene()
    net = models.NeRF_TP(num_coarse_samples=32, num_fine_samples=64, num_src_views=cases.NV).to(DEV)
    net.load_state_dict(synth.nerf_tp_state(0))
    maps = {k: sc[k].to(DEV) for k in ("plane_xz", "plane_xy", "plane_yz", "latent")}
    net.set_scene(maps["plane_xz"], maps["plane_xy"], maps["plane_yz"], maps["latent"], sc["image_wh"])
    batch = cases.neo_batch(cases.strided_rays(8))
    gbatch = {k: v.to(DEV) for k, v in batch.items()}
    pts = synth.uniform(13, "gpts", (16, 4, 3), -1.6, 1.6)           # includes points off every map (zero padding)
    gen = torch.Generator().manual_seed(4)
    uw, ul = torch.randn(cases.NV * 64, 128, generator=gen), torch.randn(cases.NV * 64, 512, generator=gen)
    with torch.enable_grad():
        cm = {k: v.clone().double().requires_grad_(True) for k, v in sc.items() if isinstance(v, torch.Tensor)}
        world_c = oracle.gather.triplane_features(pts.double(), cm["plane_xz"], cm["plane_xy"], cm["plane_yz"], batch["src_poses"].double())
        local_c = oracle.gather.pixel_aligned_features(pts.double(), cm["latent"], batch["src_poses"].double(), batch["src_focal"].double(),
                                                       batch["src_c"].double(), sc["image_wh"])
        loss = (world_c.reshape(-1, 128) * uw.double()).sum() + (local_c.reshape(-1, 512) * ul.double()).sum()
        gc = torch.autograd.grad(loss, [cm["plane_xz"], cm["plane_xy"], cm["plane_yz"], cm["latent"]])
        gm = {k: v.clone().requires_grad_(True) for k, v in maps.items()}
        world_g, local_g = training.gather_features(net, pts.to(DEV), gm["plane_xz"], gm["plane_xy"], gm["plane_yz"], gm["latent"], gbatch)
        loss_g = (world_g * uw.to(DEV)).sum() + (local_g * ul.to(DEV)).sum()
        gg = torch.autograd.grad(loss_g, [gm["plane_xz"], gm["plane_xy"], gm["plane_yz"], gm["latent"]])
    # forward: fp32 tap weights vs the float64 oracle on features of magnitude ~2 (three planes summed)
    assert max_abs(world_g, world_c.reshape(-1, 128)) < 1e-5 and max_abs(local_g, local_c.reshape(-1, 512)) < 1e-5
    w32 = oracle.gather.triplane_features(pts, sc["plane_xz"], sc["plane_xy"], sc["plane_yz"], batch["src_poses"])
    assert max_abs(world_g, w32.reshape(-1, 128)) < 2e-6
    for a, b in zip(gg, gc):
        assert a.shape == b.shape and max_abs(a, b) < 1e-5 * max(1.0, float(b.abs().max()))


def _train_net():
    net = models.NeRF_TP(num_coarse_samples=NC, num_fine_samples=NF, num_src_views=cases.NV).to(DEV)
    net.load_state_dict(synth.nerf_tp_state(0))
    sc = cases.small_scene()
    net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV), sc["image_wh"])
    return net


def test_training_forward_vs_reference_fixture(golden):
    g = golden("g8_training")
    net = _train_net()
    batch = {k: v.to(DEV) for k, v in cases.neo_batch(cases.strided_rays(NR)).items()}
    names = ("rgb", "fg_w", "bg_w", "fg_sd", "bg_sd", "bg_acc")
    for tag, randomized, white in (("det", False, False), ("white", False, True), ("rand", True, False)):
        res = net(batch, randomized, white, 0.0, 0.0, out_depth=False, seed=SEED)
        for lv in (0, 1):
            for nm, v in zip(names, res[lv]):
                ref = g["%s_%s%d" % (tag, nm, lv)]
                err = (v.cpu() - ref).abs()
                if lv == 1 and nm in ("fg_w", "bg_w", "fg_sd", "bg_sd"):
                    # per-sample rows at the fine level: a resampled position that moves by an ulp re-orders nothing but
                    # shifts a weight between neighbours; compare robustly per row
                    assert float(err.median()) < 1e-6 and float(err.quantile(0.999)) < 1e-3, (tag, nm, lv)
                else:
                    assert float(err.max()) < 1e-4, (tag, nm, lv, float(err.max()))


def test_training_forward_randomized_properties():
    net = _train_net()
    batch = {k: v.to(DEV) for k, v in cases.neo_batch(cases.strided_rays(NR)).items()}
    a = net(batch, True, False, 0.0, 0.0, out_depth=False, seed=7)
    b = net(batch, True, False, 0.0, 0.0, out_depth=False, seed=7)
    c = net(batch, True, False, 0.0, 0.0, out_depth=False, seed=8)
    d = net(batch, False, False, 0.0, 0.0, out_depth=False)
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)                                        # counter-based: same seed, same frame
    assert max_abs(a[1][3], c[1][3]) > 1e-4 and max_abs(a[1][3], d[1][3]) > 1e-4
    for res in (a, c, d):
        for lv in (0, 1):
            rgb, fg_w, bg_w, fg_sd, bg_sd, bg_acc = res[lv]
            assert bool(torch.isfinite(rgb).all()) and float(rgb.min()) > -0.01 and float(rgb.max()) < 1.01
            assert bool((fg_sd[:, 1:] >= fg_sd[:, :-1]).all()) and bool((bg_sd[:, 1:-1] <= bg_sd[:, :-2]).all())
            assert float(fg_w.min()) >= 0.0 and float(bg_w.min()) >= 0.0 and float(bg_acc.max()) <= 1.0 + 1e-5
    torch.manual_seed(0)
    e = net(batch, True, False, 0.0, 0.0, out_depth=False)              # default seed: drawn from torch's generator
    torch.manual_seed(0)
    f = net(batch, True, False, 0.0, 0.0, out_depth=False)
    assert torch.equal(e[1][0], f[1][0])


def test_training_ops_empty_inputs():
    """Zero rays through every training-side entry point: shapes kept, nothing launched, no error."""
    assert training.rand_uniform(SEED, 0, 0, 5).shape == (0, 5)
    far = torch.empty(0, 1, device=DEV)
    fg, bg = training.sample_level0(far, NC)
    assert fg.shape == bg.shape == (0, NC + 1)
    out = training.resample_u(torch.empty(0, NC + 1, device=DEV), torch.empty(0, NC + 1, device=DEV), torch.empty(0, NF, device=DEV))
    assert out.shape == (0, NC + 1 + NF)
    with torch.enable_grad():
        rgb = torch.empty(0, 8, 3, device=DEV, requires_grad=True)
        sigma = torch.empty(0, 8, 1, device=DEV, requires_grad=True)
        res = training.composite(0, rgb, sigma, torch.empty(0, 8, device=DEV), torch.empty(0, 3, device=DEV))
        assert res[0].shape == (0, 3) and res[2].shape == (0, 8)
        (res[0].sum() + res[2].sum()).backward()
        assert rgb.grad.shape == rgb.shape and sigma.grad.shape == sigma.shape
    net = models.NeRF_TP(num_coarse_samples=NC, num_fine_samples=NF, num_src_views=cases.NV).to(DEV)
    net.load_state_dict(synth.nerf_tp_state(0))
    sc = cases.small_scene()
    net.set_scene(*(sc[k].to(DEV) for k in ("plane_xz", "plane_xy", "plane_yz", "latent")), sc["image_wh"])
    batch = {k: (v.to(DEV) if k.startswith("src_") else v[:0].to(DEV)) for k, v in cases.neo_batch(cases.strided_rays(4)).items()}
    lv = net(batch, True, False, 0.0, 0.0, out_depth=False, seed=3)
    assert lv[1][0].shape == (0, 3) and lv[1][1].shape == (0, NC + 1 + NF)


@pytest.mark.parametrize("input_ch,nv", [(3, 3), (4, 3), (3, 1), (4, 2)])
def test_nerfpp_mlp_backward_vs_autograd(input_ch, nv):
    """neo_tp_mlp_train_forward / _backward against torch autograd through the oracle's NeRFPPMLP
    (oracle.mlp.nerfpp_mlp == neo360/model.py:110-158): outputs, all 18 parameter gradients and the gradients of the
    encoded points / world / local features."""
    from neo360_amd import models
    torch.manual_seed(5)
    P = 64 * 41 + 7                                   # not a multiple of the 64-row GEMM tile
    pe = 21 * input_ch
    prefix = "fg_fine_mlp." if input_ch == 3 else "bg_fine_mlp."
    sd = synth.nerf_tp_state(0)
    mlp = models.NeRFPPMLP(0, 10, 4, input_ch=input_ch, num_src_views=nv).to(DEV)
    mlp.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
    x_enc = torch.randn(nv, P, pe)
    cond = torch.randn(nv * P, 27)
    world = torch.randn(nv * P, 128) * 0.3
    local = torch.randn(nv * P, 512) * 0.3
    # ReLU kinks: a unit whose pre-activation is ~0 has derivative 0 or 1 depending on the last bit, in ANY arithmetic;
    # gradients can only be compared away from them.  Points with a pre-activation within 1e-5 of zero (fp64 forward of
    # the same network, ~3 % of the points) are dropped from the test input.
    W = {k[len(prefix):]: v.double() for k, v in sd.items() if k.startswith(prefix)}
    lin = lambda n, x: torch.nn.functional.linear(x, W[n + ".weight"], W[n + ".bias"])
    x0 = torch.cat([x_enc.reshape(-1, pe), local, world], -1).double()
    z = [lin("pts_linears.0", x0)]
    z.append(lin("pts_linears.1", z[-1].relu()))
    z.append(lin("pts_linears.2", z[-1].relu()))
    z.append(lin("pts_linears.3", torch.cat([z[-1].relu(), x0], -1)))
    h3 = z[-1].relu()
    y0 = lin("views_linear.0", torch.cat([lin("bottleneck_layer", h3), cond.double()], -1)).reshape(nv, P, -1).mean(0)
    y1 = lin("views_linear.1", y0.relu())
    near = torch.stack([zz.abs().amin(-1) for zz in z]).amin(0).reshape(nv, P).amin(0)
    near = torch.minimum(near, torch.minimum(y0.abs().amin(-1), y1.abs().amin(-1)))
    keep = near > 1e-5
    assert int(keep.sum()) > 0.9 * P
    x_enc = x_enc[:, keep].contiguous()
    sel = keep.repeat(nv)
    cond, world, local = cond[sel].contiguous(), world[sel].contiguous(), local[sel].contiguous()
    P = int(keep.sum())
    g_rgb, g_sig = torch.randn(P, 3) * 1e-3, torch.randn(P, 1) * 1e-3
    with torch.enable_grad():
        # oracle + autograd, CPU fp64 as the truth, fp32 for the scale of fp32 rounding
        def cpu(dtype):
            p = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in mlp.state_dict(prefix=prefix).items()}
            ins = [t.detach().clone().to(dtype).requires_grad_(True) for t in (x_enc, world, local)]
            rgb, sig = oracle.mlp.nerfpp_mlp(p, prefix, ins[0], cond.to(dtype), ins[1], ins[2], nv)
            (rgb * g_rgb.to(dtype)).sum().add((sig * g_sig.to(dtype)).sum()).backward()
            return rgb.detach(), sig.detach(), {k: v.grad for k, v in p.items()}, [t.grad for t in ins]
        rgb64, sig64, gp64, gi64 = cpu(torch.float64)
        gin = [t.detach().clone().to(DEV).requires_grad_(True) for t in (x_enc, world, local)]
        for p in mlp.parameters():
            p.requires_grad_(True)
            p.grad = None
        rgb, sig = training.nerfpp_mlp(mlp, gin[0], cond.to(DEV), gin[1], gin[2], nv)
        ((rgb * g_rgb.to(DEV)).sum() + (sig * g_sig.to(DEV)).sum()).backward()
    assert max_abs(rgb, rgb64) < 2e-5 and max_abs(sig, sig64) < 2e-5

    def close(got, ref64, name):
        """every entry within 2e-5 of the fp64 gradient, relative to the tensor's largest entry"""
        scale = float(ref64.abs().max()) + 1e-12
        err = float((got.detach().cpu().double() - ref64).abs().max()) / scale
        assert err < 2e-5, (name, err)
        return err

    worst = 0.0
    for name, p in mlp.named_parameters():
        worst = max(worst, close(p.grad, gp64[prefix + name], name))
    for t, r64, nm in zip(gin, gi64, ("x_enc", "world", "local")):
        worst = max(worst, close(t.grad, r64, nm))
    from conftest import record_parity
    record_parity("train_nerfpp_mlp_backward/ch%d_nv%d" % (input_ch, nv), max_rel_grad_err_vs_fp64=worst, rows=nv * P)


def test_training_step_end_to_end_gradients():
    """One differentiable pass through the whole hot path with the library's training operators - feature lookups
    (gather_features), encodings, NeRFPPMLP (nerfpp_mlp), the reference's activations, compositing (composite), an L2
    photometric loss - and its backward, against the same chain of oracle functions under torch autograd in fp64
    (the reference's training step, neo360/model.py:697-820, differentiates exactly this chain): gradients of the loss
    with respect to every MLP parameter, the three tri-planes and the latent."""
    from neo360_amd import models
    sc = cases.small_scene()
    nv, R, N = cases.NV, 24, 17
    prefix = "fg_fine_mlp."
    sd = synth.nerf_tp_state(0)
    net = models.NeRF_TP(num_coarse_samples=32, num_fine_samples=64, num_src_views=nv).to(DEV)
    net.load_state_dict(sd)
    batch = cases.neo_batch(cases.strided_rays(R))
    gb = {k: v.to(DEV) for k, v in batch.items()}
    far, _ = oracle.rays.sphere_exit_depth(batch["rays_o"], batch["rays_d"])
    t = (torch.linspace(0.05, 0.9, N)[None, :] * far).contiguous()
    pts = oracle.sampling.points_on_rays(t, batch["rays_o"], batch["rays_d"])          # (R,N,3): sample positions carry no gradient
    target = synth.uniform(31, "e2e_target", (R, 3), 0.0, 1.0)
    cam = oracle.gather.world_to_camera(pts.reshape(-1, 3), batch["src_poses"])          # (NV,P,3)
    dir_cam = oracle.gather.world_to_camera_dirs(batch["viewdirs"], batch["src_poses"])
    d_enc = oracle.encoding.pos_enc(dir_cam, 0, 4)
    cond = torch.tile(d_enc[:, None, :], (1, N, 1)).reshape(-1, d_enc.shape[-1])         # the reference's tiling (quirk Q1)
    x_enc = oracle.encoding.pos_enc(cam, 0, 10)

    def chain(world, local, mlp_fn, act_dtype):
        rgb_raw, sig_raw = mlp_fn(world, local)
        rgb = oracle.mlp.colour_activation(rgb_raw).reshape(R, N, 3)
        sigma = oracle.mlp.density_activation(sig_raw).reshape(R, N, 1)
        return rgb, sigma

    with torch.enable_grad():
        # ---- oracle, fp64 ----
        cm = {k: v.clone().double().requires_grad_(True) for k, v in sc.items() if isinstance(v, torch.Tensor)}
        pp = {k: v.double().requires_grad_(True) for k, v in sd.items() if k.startswith(prefix)}
        world_c = oracle.gather.triplane_features(pts.double(), cm["plane_xz"], cm["plane_xy"], cm["plane_yz"], batch["src_poses"].double())
        local_c = oracle.gather.pixel_aligned_features(pts.double(), cm["latent"], batch["src_poses"].double(), batch["src_focal"].double(),
                                                       batch["src_c"].double(), sc["image_wh"])
        rgb_c, sig_c = chain(world_c, local_c, lambda w, l: oracle.mlp.nerfpp_mlp(pp, prefix, x_enc.double(), cond.double(), w, l, nv), torch.float64)
        comp_c = oracle.compositing.neo_composite(rgb_c, sig_c, t.double(), batch["rays_d"].double(), True, far.double())[0]
        loss_c = ((comp_c - target.double()) ** 2).mean()
        names = sorted(pp)
        g_c = torch.autograd.grad(loss_c, [pp[k] for k in names] + [cm["plane_xz"], cm["plane_xy"], cm["plane_yz"], cm["latent"]])
        # ---- library ----
        gm = {k: sc[k].to(DEV).clone().requires_grad_(True) for k in ("plane_xz", "plane_xy", "plane_yz", "latent")}
        net.set_scene(gm["plane_xz"].detach(), gm["plane_xy"].detach(), gm["plane_yz"].detach(), gm["latent"].detach(), sc["image_wh"])
        mlp = net.fg_fine_mlp
        for p in mlp.parameters():
            p.requires_grad_(True)
            p.grad = None
        world_g, local_g = training.gather_features(net, pts.reshape(-1, 3).to(DEV), gm["plane_xz"], gm["plane_xy"], gm["plane_yz"],
                                                    gm["latent"], gb)
        rgb_g, sig_g = chain(world_g, local_g, lambda w, l: training.nerfpp_mlp(mlp, x_enc.to(DEV), cond.to(DEV), w, l, nv), torch.float32)
        comp_g = training.composite(1, rgb_g, sig_g, t.to(DEV), gb["rays_d"], far.to(DEV))[0]
        loss_g = ((comp_g - target.to(DEV)) ** 2).mean()
        params = dict(mlp.named_parameters())
        g_g = torch.autograd.grad(loss_g, [params[k[len(prefix):]] for k in names] + [gm["plane_xz"], gm["plane_xy"], gm["plane_yz"], gm["latent"]])
    assert abs(float(loss_g) - float(loss_c)) < 1e-6
    worst = 0.0
    for nm, a, b in zip(names + ["plane_xz", "plane_xy", "plane_yz", "latent"], g_g, g_c):
        scale = float(b.abs().max()) + 1e-15
        err = float((a.detach().cpu().double() - b).abs().max()) / scale
        worst = max(worst, err)
        # 5e-3 of the tensor's largest entry: a ReLU unit within an ulp of its kink contributes one row differently (see
        # test_nerfpp_mlp_backward_vs_autograd, which excludes such points and holds 2e-5); here the inputs are what they are
        assert a.shape == b.shape and err < 5e-3, (nm, err)
    from conftest import record_parity
    record_parity("train_step_end_to_end", max_rel_grad_err_vs_fp64=worst, loss_abs_err=abs(float(loss_g) - float(loss_c)))


def test_nerfpp_mlp_tapes_are_per_call():
    """A training step runs several MLP forwards before the first backward (inside / outside the sphere, coarse / fine):
    every call keeps its own activation tape.  Two calls of the same module on different inputs, one backward through
    both: the gradients equal the sum of the gradients of the two calls taken alone."""
    from neo360_amd import models
    torch.manual_seed(9)
    nv, P = 3, 700
    prefix = "fg_coarse_mlp."
    sd = synth.nerf_tp_state(0)
    mlp = models.NeRFPPMLP(0, 10, 4, input_ch=3, num_src_views=nv).to(DEV)
    mlp.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
    ins = [[torch.randn(nv, P, 63, device=DEV), torch.randn(nv * P, 27, device=DEV), torch.randn(nv * P, 128, device=DEV) * 0.3,
            torch.randn(nv * P, 512, device=DEV) * 0.3] for _ in range(2)]
    ups = [(torch.randn(P, 3, device=DEV), torch.randn(P, 1, device=DEV)) for _ in range(2)]
    params = list(mlp.parameters())

    def grads(which):
        for p in params:
            p.grad = None
        with torch.enable_grad():
            outs = [training.nerfpp_mlp(mlp, *ins[i], nv) for i in which]           # all forwards first
            loss = sum((o[0] * ups[i][0]).sum() + (o[1] * ups[i][1]).sum() for o, i in zip(outs, which))
            loss.backward()
        return [p.grad.clone() for p in params]

    for p in params:
        p.requires_grad_(True)
    both, a, b = grads([0, 1]), grads([0]), grads([1])
    for g2, ga, gb_ in zip(both, a, b):
        scale = float((ga + gb_).abs().max()) + 1e-12
        assert max_abs(g2, ga + gb_) / scale < 1e-5


def test_vanilla_mlp_backward_vs_autograd():
    """neo_vanilla_mlp_train_forward / _backward against torch autograd through the oracle's NeRFMLP (fp64): outputs, all
    24 parameter gradients, the gradients of the encoded points and of the per-ray direction encodings."""
    from neo360_amd import models
    torch.manual_seed(11)
    B, N = 600, 4          # few samples per ray: the kink filter below drops whole rays
    prefix = "fine_mlp."
    sd = synth.vanilla_state(0)
    mlp = models.NeRFMLP().to(DEV)
    mlp.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
    x_enc, d_enc = torch.randn(B, N, 63), torch.randn(B, 27)
    # drop rays with a pre-activation within 1e-5 of a ReLU kink (fp64 forward), as in test_nerfpp_mlp_backward_vs_autograd
    W = {k[len(prefix):]: v.double() for k, v in sd.items() if k.startswith(prefix)}
    lin = lambda n, x: torch.nn.functional.linear(x, W[n + ".weight"], W[n + ".bias"])
    x0 = x_enc.reshape(-1, 63).double()
    h, near = x0, torch.full((B * N,), 1e9, dtype=torch.float64)
    for i in range(8):
        z = lin("pts_linears.%d" % i, h)
        near = torch.minimum(near, z.abs().amin(-1))
        h = z.relu()
        if i == 4:
            h = torch.cat([h, x0], -1)
    cond = torch.tile(d_enc[:, None, :], (1, N, 1)).reshape(-1, 27).double()
    zv = lin("views_linear.0", torch.cat([lin("bottleneck_layer", h), cond], -1))
    near = torch.minimum(near, zv.abs().amin(-1)).reshape(B, N).amin(-1)
    keep = near > 1e-5
    assert int(keep.sum()) > 0.4 * B
    x_enc, d_enc = x_enc[keep].contiguous(), d_enc[keep].contiguous()
    B = int(keep.sum())
    g_rgb, g_sig = torch.randn(B, N, 3) * 1e-3, torch.randn(B, N, 1) * 1e-3
    with torch.enable_grad():
        p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in mlp.state_dict(prefix=prefix).items()}
        ins = [x_enc.double().requires_grad_(True), d_enc.double().requires_grad_(True)]
        rgb, sig = oracle.mlp.vanilla_mlp(p, prefix, ins[0], ins[1])
        ((rgb * g_rgb.double()).sum() + (sig * g_sig.double()).sum()).backward()
        gin = [x_enc.to(DEV).requires_grad_(True), d_enc.to(DEV).requires_grad_(True)]
        for q in mlp.parameters():
            q.requires_grad_(True)
            q.grad = None
        rgb_g, sig_g = training.nerf_mlp(mlp, gin[0], gin[1])
        ((rgb_g * g_rgb.to(DEV)).sum() + (sig_g * g_sig.to(DEV)).sum()).backward()
    assert max_abs(rgb_g, rgb.detach()) < 2e-5 and max_abs(sig_g, sig.detach()) < 2e-5
    worst = 0.0
    for name, q in mlp.named_parameters():
        ref = p[prefix + name].grad
        err = max_abs(q.grad, ref) / (float(ref.abs().max()) + 1e-12)
        worst = max(worst, err)
        assert err < 2e-5, (name, err)
    for t, r, nm in zip(gin, ins, ("x_enc", "dir_enc")):
        err = max_abs(t.grad, r.grad) / (float(r.grad.abs().max()) + 1e-12)
        worst = max(worst, err)
        assert err < 2e-5, (nm, err)
    from conftest import record_parity
    record_parity("train_vanilla_mlp_backward", max_rel_grad_err_vs_fp64=worst, rows=B * N)


def test_training_mlps_reject_wrong_shapes():
    """The training ops read rows of fixed widths through raw pointers: shape errors must surface as ValueError before the
    launch (the reference's matmuls would raise), and an unsupported gradient as NotImplementedError."""
    from neo360_amd import models
    mlp = models.NeRFPPMLP(0, 10, 4, input_ch=3, num_src_views=2).to(DEV)
    NVv, P = 2, 8
    ok = dict(x_enc=torch.randn(NVv, P, 63, device=DEV), cond=torch.randn(NVv * P, 27, device=DEV),
              world=torch.randn(NVv * P, 128, device=DEV), local=torch.randn(NVv * P, 512, device=DEV))
    rgb, sig = training.nerfpp_mlp(mlp, ok["x_enc"], ok["cond"], ok["world"], ok["local"], NVv)
    assert rgb.shape == (P, 3) and sig.shape == (P, 1)
    for key, bad in (("x_enc", torch.randn(NVv, P, 84, device=DEV)), ("cond", torch.randn(NVv * P, 32, device=DEV)),
                     ("world", torch.randn(P, 128, device=DEV)), ("local", torch.randn(NVv * P, 256, device=DEV))):
        args = dict(ok)
        args[key] = bad
        with pytest.raises(ValueError):
            training.nerfpp_mlp(mlp, args["x_enc"], args["cond"], args["world"], args["local"], NVv)
    with pytest.raises(ValueError):
        training.nerfpp_mlp(models.NeRFPPMLP(0, 10, 4, input_ch=4, num_src_views=2).to(DEV), ok["x_enc"], ok["cond"], ok["world"],
                            ok["local"], NVv)                                      # a 4-channel MLP on 63-wide encodings
    with torch.enable_grad():
        cond = ok["cond"].clone().requires_grad_(True)
        for q in mlp.parameters():
            q.requires_grad_(True)
        r, s = training.nerfpp_mlp(mlp, ok["x_enc"], cond, ok["world"], ok["local"], NVv)
        with pytest.raises(NotImplementedError):
            (r.sum() + s.sum()).backward()
    vm = models.NeRFMLP().to(DEV)
    with pytest.raises(ValueError):
        training.nerf_mlp(vm, torch.randn(4, 5, 60, device=DEV), torch.randn(4, 27, device=DEV))
    with pytest.raises(ValueError):
        training.nerf_mlp(vm, torch.randn(4, 5, 63, device=DEV), torch.randn(5, 27, device=DEV))
    # empty batches are no-ops, not errors
    r, s = training.nerf_mlp(vm, torch.zeros(0, 5, 63, device=DEV), torch.zeros(0, 27, device=DEV))
    assert r.shape == (0, 5, 3) and s.shape == (0, 5, 1)


def test_module_training_call_is_differentiable():
    """`NeRF_TP(batch, randomized, white_bkgd, near, far)` - the call of the reference's training_step
    (neo360/model.py:725-732 inside :697-820) - under autograd: same return tuple and forward values as the fused no-grad call,
    and the gradients of the reference's loss (rgb L2 on both levels + eff_distloss on the fine weights, :1246-1260) with
    respect to EVERY parameter of the four MLPs, the three tri-planes and the latent against fp64 autograd of
    oracle.neo360.render evaluated at the same fine-level sample positions (they carry no gradient; see below)."""
    sc = cases.small_scene()
    R = 256
    sd = synth.nerf_tp_state(0)
    net = models.NeRF_TP(num_coarse_samples=NC, num_fine_samples=NF, num_src_views=cases.NV).to(DEV)
    net.load_state_dict(sd)
    batch = cases.neo_batch(cases.strided_rays(R))
    gb = {k: v.to(DEV) for k, v in batch.items()}
    target = synth.uniform(77, "module_target", (R, 3), 0.0, 1.0)
    interval = 1.0 / (NC + 1 + NF)
    names = ("rgb", "fg_w", "bg_w", "fg_sd", "bg_sd", "bg_acc")

    def loss_of(levels, tgt, mask, dist):
        l = sum((((lv[0] - tgt) ** 2).sum(-1) * mask).sum() / mask.sum() for lv in levels)
        fine = levels[1]
        return l + 0.01 * (dist(fine[1] * mask[:, None], fine[3], interval) + dist(fine[2] * mask[:, None], fine[4], interval))

    gm = {k: sc[k].to(DEV).clone().requires_grad_(True) for k in ("plane_xz", "plane_xy", "plane_yz", "latent")}
    net.set_scene(gm["plane_xz"], gm["plane_xy"], gm["plane_yz"], gm["latent"], sc["image_wh"])
    # ---- forward values: fused no-grad call vs the differentiable call ----
    fused = net(gb, False, False, 0.0, 0.0, out_depth=False)
    with torch.enable_grad():
        for p in net.parameters():
            p.requires_grad_(True)
            p.grad = None
        diff = net(gb, False, False, 0.0, 0.0, out_depth=False)
        assert diff[1][0].requires_grad and diff[1][1].requires_grad
        for lv in (0, 1):
            for nm, a, b in zip(names, diff[lv], fused[lv]):
                assert a.shape == b.shape, (nm, lv)
                err = (a.detach() - b).abs()
                if lv == 1 and nm in ("fg_w", "bg_w", "fg_sd", "bg_sd"):
                    assert float(err.median()) < 1e-6 and float(err.quantile(0.999)) < 1e-3, (nm, lv)
                else:
                    assert float(err.max()) < 1e-4, (nm, lv, float(err.max()))
        # ---- oracle, fp64, autograd, AT THE LIBRARY'S FINE SAMPLE POSITIONS.  The resampled positions carry no gradient
        # (helper.py:224), but their VALUE decides which texels a sample blends: the fp64 oracle's own inverse-CDF positions
        # differ from the fp32 pipeline's by 1e-7 .. 1e-4 (conftest.check_vs_reference_noise), which moves bilinear weights -
        # and with them single entries of the feature-map gradients - by up to 1e-2.  The positions the library drew are
        # reproduced here with its own operators (bitwise what tp_render_train used) and handed to the oracle. ----
        far_g, _ = ops.intersect_sphere(gb["rays_o"], gb["rays_d"])
        fg_t0, bg_s0 = training.sample_level0(far_g, NC, None, None)
        fg_t1 = ops.resample(fg_t0, diff[0][1].detach(), NF, False)
        bg_s1 = ops.resample(bg_s0, diff[0][2].detach(), NF, True)
        sd_of = lambda t: torch.cat([0.5 * (t[..., 1:] + t[..., :-1]), t[..., -1:]], dim=-1)
        assert torch.equal(sd_of(bg_s1), diff[1][4].detach())              # really the positions of the differentiable call
        ones = torch.ones(R)
        pnames = sorted(sd)
        maps = ("plane_xz", "plane_xy", "plane_yz", "latent")

        def oracle_grads(dtype):
            cv = lambda v: v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v
            cm = {k: (cv(v).clone().requires_grad_(True) if isinstance(v, torch.Tensor) else v) for k, v in sc.items()}
            pp = {k: cv(v).clone().requires_grad_(True) for k, v in sd.items()}
            want = oracle.neo360.render(pp, {k: cv(v) for k, v in batch.items()}, cm, n_coarse=NC, n_fine=NF, white_bkgd=False,
                                        out_depth=False, fine_samples=(cv(fg_t1.cpu()), cv(bg_s1.cpu())))
            loss = loss_of(want, cv(target), cv(ones), T.eff_distloss)
            return float(loss), torch.autograd.grad(loss, [pp[k] for k in pnames] + [cm[k] for k in maps])

        loss_c, g_c = oracle_grads(torch.float64)
        _, g_r = oracle_grads(torch.float32)                 # the REFERENCE's arithmetic (fp32) on the same positions
        # ---- library ----
        loss_g = loss_of(diff, target.to(DEV), torch.ones(R, device=DEV), training.eff_distloss)
        params = dict(net.named_parameters())
        g_g = torch.autograd.grad(loss_g, [params[k] for k in pnames] + [gm[k] for k in maps])
    assert abs(float(loss_g) - loss_c) < 1e-5 * max(1.0, abs(loss_c)), (float(loss_g), loss_c)
    # The gradients of this loss are ILL-CONDITIONED in the forward pass's rounding: the fp32 oracle - the reference's own
    # arithmetic - misses its fp64 twin by up to 3.4e-3 (relative L2, the latent) / 1.1e-2 (one entry) at identical sample
    # positions (a sample within rounding of a texel boundary moves its contribution to the neighbouring texel; ReLU units
    # near their kink switch; ten octaves of positional encoding amplify the last bits of a camera-frame coordinate).  So the yardstick is that self-noise, tensor by tensor: the library may miss the fp64 gradients by
    # no more than 1.5 x what the reference's arithmetic misses them by (+ 2e-5).  Derivative correctness without the
    # forward noise is test_training_step_end_to_end's job (same intermediates on both sides: 1e-6).
    rel = lambda x, ref: (float(x.abs().max()) / (float(ref.abs().max()) + 1e-15), float(x.norm()) / (float(ref.norm()) + 1e-30))
    report, worst = {}, (0.0, "")
    for nm, a, b, r in zip(pnames + list(maps), g_g, g_c, g_r):
        assert a.shape == b.shape, nm
        a = a.detach().cpu().double()
        lib, ref, both = rel(a - b, b), rel(r.double() - b, b), rel(a - r.double(), b)
        report[nm] = (lib, ref, both)
        if lib[1] > worst[0]:
            worst = (lib[1], nm)
        assert lib[0] <= 1.5 * ref[0] + 2e-5 and lib[1] <= 1.5 * ref[1] + 2e-5, (nm, lib, ref)
    from conftest import record_parity
    record_parity("train_module_call_differentiable",
                  max_rel_l2_grad_err_vs_fp64=max(v[0][1] for v in report.values()), worst_tensor=worst[1],
                  max_rel_l2_of_the_fp32_oracle_vs_fp64=max(v[1][1] for v in report.values()),
                  max_entry_err_vs_fp64=max(v[0][0] for v in report.values()),
                  max_entry_err_of_the_fp32_oracle_vs_fp64=max(v[1][0] for v in report.values()),
                  max_rel_l2_library_vs_fp32_oracle=max(v[2][1] for v in report.values()),
                  rays=R, loss_abs_err=abs(float(loss_g) - loss_c))
    print("worst relative L2 vs fp64: library %.2e (%s); fp32 oracle %.2e; library vs fp32 oracle %.2e" % (
        worst[0], worst[1], max(v[1][1] for v in report.values()), max(v[2][1] for v in report.values())))
    for p in net.parameters():
        p.requires_grad_(False)


def test_module_training_call_same_samples_for_one_seed():
    """randomized=True: the differentiable call and the fused call draw the same stratified / inverse-CDF samples for a seed."""
    net = _train_net()
    sc = cases.small_scene()
    maps = [sc[k].to(DEV) for k in ("plane_xz", "plane_xy", "plane_yz", "latent")]
    net.set_scene(*maps, sc["image_wh"])
    gb = {k: v.to(DEV) for k, v in cases.neo_batch(cases.strided_rays(NR)).items()}
    fused = net(gb, True, False, 0.0, 0.0, out_depth=False, seed=SEED)
    with torch.enable_grad():
        for p in net.parameters():
            p.requires_grad_(True)
        diff = net(gb, True, False, 0.0, 0.0, out_depth=False, seed=SEED)
    assert torch.equal(diff[0][3], fused[0][3]) and torch.equal(diff[0][4], fused[0][4])          # level-0 rows: bit-identical
    assert float((diff[1][3] - fused[1][3]).abs().median()) < 1e-6                                   # level 1: same draws on ~equal weights
    assert max_abs(diff[0][0].detach(), fused[0][0]) < 1e-4
    del maps
    import gc
    gc.collect()
    with torch.enable_grad(), pytest.raises(Exception, match="scene tensors"):
        net(gb, True, False, 0.0, 0.0, out_depth=False, seed=SEED)                                     # the maps are gone
