"""GPU: the scene axis of the inference path - source-view counts 1..8 and feature maps from 2 x 2 texels up - through every point
evaluator, the fused NeO-360 render with and without background culling, the scene encoder's pillar stage forward and backward,
and the training lookups.  Cases, references and bounds: tests/view_map_cases.py (checked on the CPU by
tests/test_view_map_cases_cpu.py); every comparison is per entry against fp64, the worst share of a bound per case goes to the
parity report under view_map_sweep/.  References are evaluated once per case and shared by the kernel variants; the GPU outputs of
a (variant, scene) are kept for the variant-agreement test."""
import pytest
import torch

import alongray_cases as A
import oracle
import view_map_cases as V
from conftest import max_abs, record_parity
from neo360_amd import encoder, models, ops, synth, training

pytestmark = pytest.mark.gpu
DEV = "cuda"
_NEO_OUT, _PIX_OUT = {}, {}
SCENE_IDS = range(len(V.SCENES))


def _dev(b):
    return {k: v.to(DEV) for k, v in b.items()}


def _scene_id(s):
    nv, (ph, pw), (lh, lw) = V.SCENES[s]
    return "nv%d-%dx%d-%dx%d" % (nv, ph, pw, lh, lw)


def _tp_net(s, variant="f16x3", state=None, samples=(16, 24)):
    nv = V.SCENES[s][0]
    sc = V.scene_of(s)
    net = models.NeRF_TP(num_coarse_samples=samples[0], num_fine_samples=samples[1], num_src_views=nv).to(DEV)
    net.precision = variant.split("-")[0]
    net.load_state_dict(synth.nerf_tp_state(0) if state is None else state)
    net.set_scene(sc["plane_xz"].to(DEV), sc["plane_xy"].to(DEV), sc["plane_yz"].to(DEV), sc["latent"].to(DEV), sc["image_wh"],
                  preproject={"pp1": True, "pp2": 2, "noproj": False}.get(variant.split("-")[-1]))       # None: the default (3)
    return net


def _neo_outputs(variant, s):
    """{P: (inside (R,N,4), outside (R,N,4))} of one evaluator variant on every case of scene s, on the host."""
    if (variant, s) not in _NEO_OUT:
        net = _tp_net(s, variant)
        out = {}
        for t, P in V.CASES:
            if t != s:
                continue
            c = V.point_case(s, P)
            gb, far = _dev(c["batch"]), c["far"].to(DEV)
            fg = net.eval_mlp(V.FG_SLOT, gb, c["t_in"].to(DEV), far=far, chunk=c["chunk"]).cpu()
            bg = net.eval_mlp(V.BG_SLOT, gb, c["s_out"].to(DEV), far=far, chunk=c["chunk"]).cpu()
            out[P] = (fg, bg)
        net.close()
        _NEO_OUT[(variant, s)] = out
    return _NEO_OUT[(variant, s)]


def _pix_outputs(precision, preproject, s):
    if (precision, preproject, s) not in _PIX_OUT:
        nv = V.SCENES[s][0]
        sc = V.scene_of(s)
        net = models.PixelNeRF(num_src_views=nv).to(DEV)
        net.precision = precision
        net.preproject = preproject
        net.load_state_dict(synth.pixelnerf_state(0))
        net.set_scene(sc["latent"].to(DEV), sc["image_wh"])
        out = {}
        for t, P in V.CASES:
            if t != s:
                continue
            c = V.point_case(s, P)
            out[P] = net.eval_mlp(V.PIX_SLOT, _dev(c["batch"]), c["t_in"].to(DEV), chunk=c["chunk"]).cpu()
        net.close()
        _PIX_OUT[(precision, preproject, s)] = out
    return _PIX_OUT[(precision, preproject, s)]


def _judge(label, checks):
    record_parity("view_map_sweep/" + label, **A.summarize(checks))
    print(label, {k: "%.2e of %.2e (fp32 oracle %.2e)" % (v["err"], v["bound"], v["fp32"]) for k, v in checks.items()})
    return checks


def _assert_all(judged):
    for label, checks in judged:
        A.assert_inside(checks, label)


# ---- point evaluators ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SCENE_IDS, ids=_scene_id)
@pytest.mark.parametrize("variant", V.NEO_VARIANTS)
def test_neo360_evaluators(variant, s):
    """NeRF_TP.eval_mlp on a slot inside and a slot outside the sphere, every case of the scene, per entry against fp64."""
    got = _neo_outputs(variant, s)
    judged = []
    for P, (fg, bg) in got.items():
        c = V.point_case(s, P)
        assert fg.shape == bg.shape == (c["R"], c["N"], 4)
        fg64, bg64 = V.neo_reference(s, P)
        fg32, bg32 = V.neo_reference(s, P, torch.float32)
        for name, g, a, b in (("inside", fg, fg64, fg32), ("outside", bg, bg64, bg32)):
            label = "neo360/%s/%s/P%d/%s" % (variant, _scene_id(s), P, name)
            judged.append((label, _judge(label, V.eval_checks(g, a, b))))
    _assert_all(judged)


@pytest.mark.parametrize("s", SCENE_IDS, ids=_scene_id)
@pytest.mark.parametrize("precision,preproject", V.PIX_VARIANTS, ids=["%s-%s" % (p, "pre" if q else "noproj") for p, q in V.PIX_VARIANTS])
def test_pixelnerf_evaluators(precision, preproject, s):
    got = _pix_outputs(precision, preproject, s)
    judged = []
    for P, g in got.items():
        c = V.point_case(s, P)
        assert g.shape == (c["R"], c["N"], 4)
        label = "pixelnerf/%s-%s/%s/P%d" % (precision, "pre" if preproject else "noproj", _scene_id(s), P)
        judged.append((label, _judge(label, V.eval_checks(g, V.pix_reference(s, P), V.pix_reference(s, P, torch.float32)))))
    _assert_all(judged)


@pytest.mark.parametrize("s", SCENE_IDS, ids=_scene_id)
def test_variants_agree(s):
    """Every pair of evaluator variants on every case of the scene: the bounds of test_preprojection_is_a_reassociation."""
    worst = dict(rgb=0.0, sigma=0.0)
    bad = []
    families = [("neo360", [(v, _neo_outputs(v, s)) for v in V.NEO_VARIANTS]),
                ("pixelnerf", [("%s-%s" % (p, q), _pix_outputs(p, q, s)) for p, q in V.PIX_VARIANTS])]
    for family, outs in families:
        for i, (va, a) in enumerate(outs):
            for vb, b in outs[i + 1:]:
                for P in a:
                    xs, ys = (a[P], b[P]) if family == "neo360" else ((a[P],), (b[P],))
                    for x, y in zip(xs, ys):
                        d_rgb, d_sigma = max_abs(x[..., :3], y[..., :3]), max_abs(x[..., 3], y[..., 3])
                        worst["rgb"], worst["sigma"] = max(worst["rgb"], d_rgb), max(worst["sigma"], d_sigma)
                        if not (d_rgb < V.AGREE_RGB and d_sigma < V.AGREE_SIGMA):
                            bad.append((family, va, vb, P, d_rgb, d_sigma))
    record_parity("view_map_sweep/variants_agree/" + _scene_id(s), max_rgb=worst["rgb"], max_sigma=worst["sigma"],
                  bound_rgb=V.AGREE_RGB, bound_sigma=V.AGREE_SIGMA)
    print(_scene_id(s), "largest disagreement between two variants: rgb %.2e, sigma %.2e" % (worst["rgb"], worst["sigma"]))
    assert not bad, bad


# ---- fused render ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", V.RENDER_SCENES, ids=_scene_id)
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_fused_render_is_the_stage_chain_and_culling_keeps_its_contract(precision, s):
    """net(batch, out_depth=True) against the chain of stage calls (the last lines of test_pipeline_stage_by_stage), then the
    cull_background contract of test_gpu_cull_background.py against the un-culled call on the same scene, on a mixed frame."""
    from test_gpu_cull_background import _assert_contract, _assert_mixed, _call, _culled_set
    NC, NF = V.RENDER_SAMPLES
    net = _tp_net(s, precision, state=V.render_state(s), samples=V.RENDER_SAMPLES)
    batch = V.render_batch(s)
    gb = _dev(batch)
    o, d = batch["rays_o"], batch["rays_d"]
    far_c, _ = oracle.rays.sphere_exit_depth(o, d)
    far_g, ok = ops.intersect_sphere(gb["rays_o"], gb["rays_d"])
    assert bool(ok.all()) and max_abs(far_g.cpu(), far_c) < 1e-6
    fg_t, _ = oracle.sampling.neo_fg_level0(o, d, NC, torch.full_like(far_c, 1e-4), far_c)
    bg_s, _, _ = oracle.sampling.neo_bg_level0(o, d, NC, far_c, 3.0)
    fg0 = net.eval_mlp(0, gb, fg_t.to(DEV), far=far_g)
    bg0 = net.eval_mlp(2, gb, bg_s.to(DEV), far=far_g)
    cf = ops.composite(1, fg0, fg_t.to(DEV), gb["rays_d"], far_g)
    cb = ops.composite(2, bg0, bg_s.to(DEV))
    fg_t1 = ops.resample(fg_t.to(DEV), cf["weights"], NF)
    bg_s1 = ops.resample(bg_s.to(DEV), cb["weights"], NF, descending=True)
    assert fg_t1.shape == bg_s1.shape == (V.RENDER_RAYS, NC + 1 + NF)
    fg1 = net.eval_mlp(1, gb, fg_t1, far=far_g)
    bg1 = net.eval_mlp(3, gb, bg_s1, far=far_g)
    cf1 = ops.composite(1, fg1, fg_t1, gb["rays_d"], far_g)
    cb1 = ops.composite(2, bg1, bg_s1)
    rgb_g = cf1["rgb"] + cf1["bg_lambda"] * cb1["rgb"]
    depth_g = cf1["depth"] + cf1["bg_lambda"].squeeze(-1) * cb1["depth"]
    res = net(gb, False, False, 0.0, 0.0, out_depth=True)
    net.check_flags()
    assert bool(torch.isfinite(res[1][0]).all()) and bool(torch.isfinite(res[1][5]).all())
    d_rgb, d_depth = max_abs(res[1][0], rgb_g), max_abs(res[1][5], depth_g)
    record_parity("view_map_sweep/render/%s/%s" % (precision, _scene_id(s)), fused_vs_chain_rgb=d_rgb, fused_vs_chain_depth=d_depth)
    assert d_rgb < 1e-6 and d_depth < 1e-6
    full = _call(net, gb, None)
    _assert_mixed(_culled_set(full, V.CULL_EPS))
    got = _call(net, gb, V.CULL_EPS)
    _assert_contract(net, full, got, V.CULL_EPS)
    net.close()


# ---- pillar stage ----------------------------------------------------------------------------------------------------------------
def _pillar_id(i):
    nv, (lh, lw), g = V.PILLAR[i]
    return "nv%d-%dx%d-g%dx%dx%d" % (nv, lh, lw, g[0], g[1], g[2])


def _enc(c, precision):
    enc = encoder.GridEncoder(grid_size=c["grid"]).to(DEV)
    enc.precision = precision
    enc.on_range = "raise"
    enc.load_state_dict(c["params"], strict=False)
    return enc


@pytest.mark.parametrize("i", range(len(V.PILLAR)), ids=_pillar_id)
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_pillar_forward(precision, i):
    """GridEncoder.floorplans per entry against fp64; the differentiable forward is bitwise floorplans."""
    c = V.pillar_case(i)
    enc = _enc(c, precision)
    args = (c["poses"].to(DEV), c["focal"].to(DEV), c["centre"].to(DEV), c["image_wh"])
    lat = c["latent"].to(DEV)
    got = enc.floorplans(lat, *args)
    assert enc.last_precision_used == precision
    label = "pillar/%s/%s" % (precision, _pillar_id(i))
    checks = _judge(label, V.plan_checks(got, V.pillar_reference(i), V.pillar_reference(i, torch.float32)))
    with torch.enable_grad():
        again = enc.floorplans_train(lat.clone().requires_grad_(True), *args)
    for a, b in zip(again, got):
        assert a.requires_grad and torch.equal(a.detach(), b)
    A.assert_inside(checks, label)
    enc.close()


_PILLAR_G = {}


def _pillar_oracle_grads(i, cot):
    from test_gpu_encoder_training import _oracle_grads
    if i not in _PILLAR_G:
        c = V.pillar_case(i)
        a = (c["params"], c["scene"], c["poses"], c["focal"], c["centre"], c["grid"], cot)
        with torch.enable_grad():
            _PILLAR_G[i] = (_oracle_grads(*a, torch.float64), _oracle_grads(*a, torch.float32))
    return _PILLAR_G[i]


@pytest.mark.parametrize("i", V.PILLAR_GRAD, ids=_pillar_id)
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_pillar_gradients(precision, i):
    """All 18 parameter gradients and the latent gradient under the rule of test_gradients_vs_fp64_oracle, unchanged: per tensor,
    relative max and relative L2 within 1.5 x what the fp32 oracle misses fp64 by, plus the forward's share (the fp64 backward fed
    the library's own tape against plain fp64), plus 2e-5; a scorer head's bias gradient is exactly zero and is held to 1e-4."""
    from test_gpu_encoder_training import HEAD_BIAS, NAMES, _cotangents, _library_grads, _oracle_grads, _rel, _tape_parts
    c = V.pillar_case(i)
    nv, grid = c["nv"], c["grid"]
    cot = _cotangents(grid, nv)
    g64, g32 = _pillar_oracle_grads(i, cot)
    enc = _enc(c, precision)
    with torch.enable_grad():
        fps, lib = _library_grads(enc, c["scene"], c["poses"], c["focal"], c["centre"], cot)
        tape = [t.detach().cpu() for t in _tape_parts(fps[0], grid, nv)]
        gt = _oracle_grads(c["params"], c["scene"], c["poses"], c["focal"], c["centre"], grid, cot, torch.float64, tape=tape)
    worst, bad = {}, []
    for n in NAMES + ["latent"]:
        a, b, r = lib[n], g64[n], g32[n]
        assert a.shape == b.shape, n
        assert bool(torch.isfinite(a).all()), n
        if n in HEAD_BIAS:
            assert float(a.abs().max()) <= 1e-4, (n, float(a[0]))
            continue
        mine, ref, fwd = _rel(a.cpu().double() - b, b), _rel(r.double() - b, b), _rel(gt[n] - b, b)
        worst[n] = (mine, ref, fwd)
        if not (mine[0] <= 1.5 * ref[0] + fwd[0] + 2e-5 and mine[1] <= 1.5 * ref[1] + fwd[1] + 2e-5):
            bad.append((n, mine, ref, fwd))
    share = {n: max(m[k] / (1.5 * r[k] + f[k] + 2e-5) for k in (0, 1)) for n, (m, r, f) in worst.items()}
    w = max(share, key=share.get)
    record_parity("view_map_sweep/pillar_grad/%s/%s" % (precision, _pillar_id(i)), worst_share_of_bound=float("%.3g" % share[w]),
                  worst_tensor=w, rel_max=worst[w][0][0], rel_l2=worst[w][0][1], fp32_oracle_rel_max=worst[w][1][0],
                  fp32_oracle_rel_l2=worst[w][1][1])
    # the derivative alone: the oracle's backward at the library's taped h1, h2, L and scores agrees to 1e-5 relative
    alone = {n: _rel(lib[n].cpu().double() - gt[n], gt[n])[1] for n in NAMES + ["latent"] if n not in HEAD_BIAS}
    print(_pillar_id(i), precision, "worst share of the gradient rule %.3f (%s); backward alone, worst relative L2 %.2e"
          % (share[w], w, max(alone.values())))
    assert not bad, bad
    assert max(alone.values()) <= 1e-5, alone
    enc.close()


# ---- training lookups ------------------------------------------------------------------------------------------------------------
def _lookup_id(i):
    nv, _, (lh, lw) = V.LOOKUP_SCENES[i]
    return "nv%d-%dx%d" % (nv, lh, lw)


@pytest.mark.parametrize("i", range(len(V.LOOKUP_SCENES)), ids=_lookup_id)
def test_training_lookups(i):
    """training.gather_features and training.gather_map forward and backward on maps of 4 and 35 texels per view, against fp64
    autograd of oracle.gather."""
    c = V.lookup_case(i)
    sc, nv = c["scene"], c["nv"]
    net = models.NeRF_TP(num_coarse_samples=16, num_fine_samples=24, num_src_views=nv).to(DEV)
    net.set_scene(*(sc[k].to(DEV) for k in V.MAPS), sc["image_wh"])
    gb = _dev(c["batch"])
    up = {k: v.to(DEV) for k, v in c["up"].items()}
    pts = c["pts"].to(DEV)
    with torch.enable_grad():
        gm = {k: sc[k].to(DEV).clone().requires_grad_(True) for k in V.MAPS}
        world, local = training.gather_features(net, pts, gm["plane_xz"], gm["plane_xy"], gm["plane_yz"], gm["latent"], gb)
        grads = torch.autograd.grad((world * up["world"]).sum() + (local * up["local"]).sum(), [gm[k] for k in V.MAPS])
        m = c["gmap"].to(DEV).requires_grad_(True)
        rows = training.gather_map(net, m, pts, gb)
        (g_map,) = torch.autograd.grad((rows * up["map"]).sum(), m)
    got = dict(world=world.detach(), local=local.detach(), map_rows=rows.detach(), g_map=g_map)
    got.update({"g_" + k: g for k, g in zip(V.MAPS, grads)})
    label = "lookups/" + _lookup_id(i)
    checks = _judge(label, V.lookup_checks(got, V.lookup_reference(i), V.lookup_reference(i, torch.float32)))
    A.assert_inside(checks, label)
    net.close()
