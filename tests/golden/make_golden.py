"""Generates tests/golden/*.npz by running the REFERENCE ITSELF (imported from
/root/reference under import stubs, see _ref_loader.py) on the seeded inputs of
cases.py.  Build-container only; the fixtures (expected outputs) are committed,
the reference never travels.

    python tests/golden/make_golden.py            # regenerate everything
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

import _ref_loader as ref  # noqa: E402
import cases  # noqa: E402
from neo360_amd import synth  # noqa: E402

torch.set_grad_enabled(False)


def save(name, **arrays):
    out = {}
    for k, v in arrays.items():
        out[k] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-28s %7.1f KB  %s" % (name, os.path.getsize(path) / 1024, {k: a.shape for k, a in out.items()}))


# ---------------------------------------------------------------------------------
# reference module builders
# ---------------------------------------------------------------------------------

def ref_vanilla(state):
    M = ref.load("models.vanilla_nerf.model")
    net = M.NeRF()
    net.load_state_dict(state, strict=True)
    return net.eval()


class _FakeEncoder(torch.nn.Module):
    """Stands in for GridEncoder (outside the hot path): returns fixed tri-planes and
    exposes the reference's real SpatialEncoder with a preset latent."""

    def __init__(self, scene, spatial):
        super().__init__()
        self.scene = scene
        self.spatial_encoder = spatial
        self.latent_size = 512

    def forward(self, *a, **k):
        return self.scene["plane_xz"], self.scene["plane_xy"], self.scene["plane_yz"]


def ref_nerf_tp(state, scene, nv=cases.NV):
    M = ref.load("models.neo360.model")
    E = ref.load("models.neo360.encoder_pn")
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        net = M.NeRF_TP(num_src_views=nv)
    spatial = E.SpatialEncoder.__new__(E.SpatialEncoder)
    torch.nn.Module.__init__(spatial)
    spatial.index_interp, spatial.index_padding = "bilinear", "zeros"
    spatial.register_buffer("latent", scene["latent"], persistent=False)
    Hf, Wf = scene["latent"].shape[-2:]
    ls = torch.tensor([float(Wf), float(Hf)])
    spatial.register_buffer("latent_scaling", ls / (ls - 1) * 2.0, persistent=False)
    net.encoder = _FakeEncoder(scene, spatial)
    missing = net.load_state_dict(state, strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("encoder")], missing
    assert not missing.unexpected_keys, missing
    return net.eval()


# ---------------------------------------------------------------------------------
# G1 ray generation   (datasets/ray_utils.py)
# ---------------------------------------------------------------------------------

def g1_raygen():
    RU = ref.load("datasets.ray_utils")
    out = {}
    for tag, (H, W) in (("s", (32, 32)), ("f", (480, 640))):
        focal = 0.8 * W
        dirs = RU.get_ray_directions(H, W, focal)
        for pi, az in enumerate((10.0, 130.0, 250.0)):
            c2w = synth.look_at_origin(az, 0.6 + 0.1 * pi, 0.3 - 0.2 * pi)[:3, :4]
            ro, vd, rd, rad = RU.get_rays(dirs.clone(), c2w, output_view_dirs=True, output_radii=True)
            if tag == "f":  # corners, centre, last rows: keep the fixture small
                rows = torch.tensor([0, 1, 239, 240, 477, 478, 479])
                idx = (rows[:, None] * W + torch.arange(0, W, 7)[None, :]).reshape(-1)
                ro, vd, rd, rad = ro[idx], vd[idx], rd[idx], rad[idx]
                out["idx_%s" % tag] = idx
            out["o_%s%d" % (tag, pi)] = ro
            out["v_%s%d" % (tag, pi)] = vd
            out["d_%s%d" % (tag, pi)] = rd
            out["r_%s%d" % (tag, pi)] = rad
    save("g1_raygen", **out)


# ---------------------------------------------------------------------------------
# G2 AABB hit masks   (datasets/ray_utils.py:17-68, neo360/helper.py:359-373)
# ---------------------------------------------------------------------------------

def g2_aabb():
    RU = ref.load("datasets.ray_utils")
    H = ref.load("models.neo360.helper")
    boxes, o, d = cases.aabb_cases()
    out = {}
    nears, fars = [], []
    for bi, b in enumerate(boxes):
        hit, tmin, tmax = RU.bbox_intersection_batch(b, o.copy(), d.copy())
        hit2, _, _ = H.bbox_intersection_batch(b, o.copy(), d.copy())
        assert np.array_equal(hit, hit2)
        out["hit%d" % bi] = hit.astype(np.uint8)
        out["tmin%d" % bi] = tmin
        out["tmax%d" % bi] = tmax
        nears.append(torch.Tensor(tmin[:, None]))
        fars.append(torch.Tensor(tmax[:, None]))
    # multi-box merge with 0 sentinel (helper.py:359-373), restated inline from the reference's loop
    all_near = torch.zeros_like(nears[0])
    all_far = torch.zeros_like(fars[0])
    for near, far in zip(nears, fars):
        all_near = torch.where((all_near == 0) | (near == 0), torch.maximum(near, all_near), torch.minimum(near, all_near))
        all_far = torch.where((all_far == 0) | (far == 0), torch.maximum(far, all_far), torch.minimum(far, all_far))
    out["merged_mask"] = ((all_near != 0) & (all_far != 0)).numpy().astype(np.uint8)
    # oriented boxes through the reference's own sample_rays_in_bbox / get_object_rays_in_bbox (helper.py:348-373)
    RTs, wo, wd = cases.oriented_box_cases()
    near, far, mask = H.sample_rays_in_bbox(RTs, wo.copy(), wd.copy())
    out.update(ob_near=near, ob_far=far, ob_mask=mask.numpy().astype(np.uint8))
    for bi in range(len(RTs["R"])):
        single = {"R": RTs["R"][bi], "T": RTs["T"][bi], "s": RTs["s"][bi]}
        hit, _, _ = H.get_object_rays_in_bbox(wo.copy(), wd.copy(), single)
        out["ob_hit%d" % bi] = hit.numpy().astype(np.uint8)
    save("g2_aabb", **out)


# ---------------------------------------------------------------------------------
# G3 per-stage
# ---------------------------------------------------------------------------------

def g3_stages():
    HN = ref.load("models.neo360.helper")
    HV = ref.load("models.vanilla_nerf.helper")
    ENC = ref.load("models.neo360.encoder_tp_fusion_conv")
    M = ref.load("models.neo360.model")
    out = {}
    # pos_enc, 3/4/3 channels
    x3 = synth.uniform(11, "pe3", (257, 3), -1.7, 1.7)
    x4 = synth.uniform(11, "pe4", (129, 4), -1.0, 1.0)
    out["pe3"] = HN.pos_enc(x3, 0, 10)
    out["pe4"] = HN.pos_enc(x4, 0, 10)
    out["pe3v"] = HV.pos_enc(x3, 0, 4)
    # sphere intersection + inverted-sphere points
    rays = cases.strided_rays(96)
    out["far"] = HN.intersect_sphere(rays["rays_o"], rays["rays_d"])
    inv_r = torch.flip(torch.linspace(0, 1, 33), dims=[-1])[None].repeat(96, 1).contiguous()
    out["outside"] = HN.depth2pts_outside(rays["rays_o"], rays["rays_d"], inv_r)
    # level-0 samplers
    near = torch.full((96, 1), 1e-4)
    t_fg, p_fg = HN.sample_along_rays(rays["rays_o"], rays["rays_d"], 32, near, out["far"], False, False, True)
    s_bg, p_bg, l_bg = HN.sample_along_rays(rays["rays_o"], rays["rays_d"], 32, near, out["far"], False, False,
                                             False, far_uncontracted=3)
    out.update(fg0_t=t_fg, fg0_p=p_fg, bg0_s=s_bg, bg0_p=p_bg, bg0_lin=l_bg)
    tv, pv = HV.sample_along_rays(rays["rays_o"], rays["viewdirs"], 64, 0.2, 3.0, False, False)
    out.update(v0_t=tv[:2], v0_p=pv[:2])
    # inverse-CDF sampling
    pc = cases.pdf_cases()
    for tag, (bins, w) in pc.items():
        out["pdf_" + tag] = HN.sorted_piecewise_constant_pdf(bins, w, 128, False)
    out["pdf_asc_v"] = HV.sorted_piecewise_constant_pdf(pc["asc"][0], pc["asc"][1], 128, False)
    # compositing
    rgb, sigma, t, dirs, far = cases.composite_case()
    names = ("rgb", "acc", "w", "lam", "depth")
    for nm, v in zip(names, HN.volumetric_rendering(rgb, sigma, t, dirs, False, True, t_far=far, out_depth=True)):
        out["cfg_" + nm] = v
    t_desc = torch.flip(t / t.max(), dims=[-1]).contiguous()
    for nm, v in zip(names, HN.volumetric_rendering(rgb, sigma, t_desc, dirs, False, False, out_depth=True)):
        if v is not None:
            out["cbg_" + nm] = v
    for nm, v in zip(("rgb", "acc", "w", "depth"), HV.volumetric_rendering(rgb, sigma, t, dirs * 1.3, True)):
        out["cv_" + nm] = v
    # feature lookups: tri-planes and pixel-aligned latents, including out-of-range points
    scene = cases.small_scene()
    poses, focal, centre = synth.source_views(cases.NV, *cases.IMG_WH)
    pts = synth.uniform(13, "gpts", (16, 4, 3), -1.6, 1.6)
    out["triplane"] = ENC.index_grid(pts, scene["plane_xz"], scene["plane_xy"], scene["plane_yz"], poses,
                                     src_views_num=cases.NV)
    net = ref_nerf_tp(synth.nerf_tp_state(1), scene)
    net.image_shape = torch.Tensor([cases.IMG_WH[0], cases.IMG_WH[1]])
    net.latent_size = 512
    loc, cam = net.get_local_feats(pts, poses, focal, centre, src_views_num=cases.NV)
    out["local"] = loc
    out["cam"] = cam
    # NeRFPPMLP, NV = 1 and 3
    for nv in (1, 3):
        P = 50
        mlp = M.NeRFPPMLP(0, 10, 4, num_src_views=nv)
        sd = synth.nerfpp_mlp_state(21 + nv, "")
        mlp.load_state_dict(sd)
        x = synth.uniform(31, "mlp_x%d" % nv, (nv, P, 63), -1, 1)
        cond = synth.uniform(31, "mlp_c%d" % nv, (nv * P, 27), -1, 1)
        world = synth.normal(31, "mlp_w%d" % nv, (nv * P, 128), 0.3)
        local = synth.normal(31, "mlp_l%d" % nv, (nv * P, 512), 0.3)
        r, s = mlp(x, cond, world, local, combine_inner_dims=(nv, P))
        out["mlp%d_rgb" % nv] = r
        out["mlp%d_sigma" % nv] = s
    # vanilla NeRFMLP
    MV = ref.load("models.vanilla_nerf.model")
    vm = MV.NeRFMLP(0, 10, 4)
    vm.load_state_dict(synth.vanilla_mlp_state(41, ""))
    xe = synth.uniform(43, "vmlp_x", (6, 11, 63), -1, 1)
    ce = synth.uniform(43, "vmlp_c", (6, 27), -1, 1)
    r, s = vm(xe, ce)
    out["vmlp_rgb"], out["vmlp_sigma"] = r, s
    save("g3_stages", **out)


# ---------------------------------------------------------------------------------
# G4 / G5 end to end
# ---------------------------------------------------------------------------------

def g3_pdf_noise():
    """The reference's own rounding in the inverse-CDF sampler (neo360/helper.py:174-215) on the rows of
    cases.pdf_cases(): the same function evaluated in fp64.  With DEscending bins (the background branch) every sample
    interpolates across the whole range and one ulp of the fp32 cdf moves it by up to ~1e-4: the GPU position bounds of
    tests/test_gpu_stages.py are stated against this fixture."""
    HN = ref.load("models.neo360.helper")
    out = {}
    for tag, (bins, w) in cases.pdf_cases().items():
        r32 = HN.sorted_piecewise_constant_pdf(bins, w, 128, False)
        r64 = HN.sorted_piecewise_constant_pdf(bins.double(), w.double(), 128, False)
        assert r64.dtype == torch.float64
        out["noise_pdf_" + tag] = (r32.double() - r64).abs().float()      # per sample; the tests use the per-row maximum
        print("pdf", tag, "max |ref32 - ref64| = %.3e" % float(out["noise_pdf_" + tag].max()))
    save("g3_pdf_noise", **out)


def g4_vanilla():
    out = {}
    for tag, gain in (("", 1.0), ("_sharp", 8.0)):
        net = ref_vanilla(synth.vanilla_state(0, density_gain=gain))
        rays = cases.crop_rays(32, 32)  # config 1: 32x32 crop
        res = net(rays, False, False, 0.2, 3.0)
        for lv in (0, 1):
            out["rgb%d%s" % (lv, tag)] = res[lv][0]
            out["acc%d%s" % (lv, tag)] = res[lv][1]
            out["depth%d%s" % (lv, tag)] = res[lv][2]
    net = ref_vanilla(synth.vanilla_state(0))
    res = net(cases.strided_rays(200), False, True, 0.2, 3.0)  # white background, ragged count
    out["rgb1_white"], out["depth1_white"] = res[1][0], res[1][2]
    save("g4_vanilla", **out)


def _neo_inputs(n_rays, nv, full):
    """(scene, batch): the small fixture scene, or the BASELINE C3 configuration at full size (cases.full_*);
    full = "b1".."b4": the additional full-size chunks of cases.FULL_B (their own pose / strip / view count)."""
    if isinstance(full, str):
        assert cases.FULL_B[full]["nv"] == nv
        return cases.full_case(full, n_rays)
    if full:
        return cases.full_scene(nv=nv), cases.full_batch(n_rays, nv=nv)
    return cases.small_scene(nv=nv), cases.neo_batch(cases.strided_rays(n_rays), nv=nv)


def g4_neo(tag, n_rays, chunk, n_coarse=128, n_fine=256, gain=1.0, nv=cases.NV, full=False):
    scene, batch = _neo_inputs(n_rays, nv, full)
    net = ref_nerf_tp(synth.nerf_tp_state(0, density_gain=gain), scene, nv=nv)
    net.num_coarse_samples, net.num_fine_samples = n_coarse, n_fine
    per_ray = ("rays_o", "rays_d", "viewdirs")
    acc = {k: [] for k in ("rgb0", "rgb1", "fg1", "bg1", "fgacc1", "lam1", "depth0", "depth1")}
    for i in range(0, n_rays, chunk):
        part = {k: (v[i:i + chunk] if k in per_ray else v) for k, v in batch.items()}
        res = net(part, False, False, 0.0, 0.0, out_depth=True)
        acc["rgb0"].append(res[0][0]); acc["depth0"].append(res[0][5])
        acc["rgb1"].append(res[1][0]); acc["fg1"].append(res[1][1]); acc["bg1"].append(res[1][2])
        acc["fgacc1"].append(res[1][3]); acc["lam1"].append(res[1][4]); acc["depth1"].append(res[1][5])
    save("g4_neo_" + tag, **{k: torch.cat(v, 0) for k, v in acc.items()})


class _MarginProbe:
    """Records, for every call of the reference's inverse-CDF sampler (neo360/helper.py:174-215) while active, the
    per-ray distance between its quantiles u and the interior values of ITS OWN cdf (captured from its torch.cumsum):
    margin = min_ij |u_j - cdf_i|.  With DEscending bins (the background branch) the sampler is discontinuous at
    every u_j = cdf_i: bin0 / bin1 are always the first / last bin, so the interpolation weight jumps from 1 to 0 and
    one sample crosses the whole range.  A ray whose margin is a few ulps of the cdf changes under ANY faithful
    re-evaluation of the coarse level; the tests use the margin to recognise such rays (flip-prone rays)."""

    def __init__(self, helper_module):
        self.h = helper_module
        self.orig = helper_module.sorted_piecewise_constant_pdf
        self.margins = []
        self.cdfs = []                # the interior cdf values of every call (float64 copies): g4_neo_noise compares them across runs

    def __enter__(self):
        probe = self

        def wrapped(bins, weights, num_samples, randomized, float_min_eps=2 ** -32):
            real_cumsum, seen = torch.cumsum, []

            def spy(*a, **k):
                out = real_cumsum(*a, **k)
                seen.append(out)
                return out

            torch.cumsum = spy
            try:
                res = probe.orig(bins, weights, num_samples, randomized, float_min_eps)
            finally:
                torch.cumsum = real_cumsum
            inner = torch.fmin(torch.ones_like(seen[0]), seen[0]).double()
            u = torch.linspace(0.0, 1.0 - float_min_eps, num_samples).double()
            probe.margins.append((u[None, None, :] - inner[:, :, None]).abs().reshape(inner.shape[0], -1).min(dim=-1).values.float())
            probe.cdfs.append(inner.clone())
            return res

        self.h.sorted_piecewise_constant_pdf = wrapped
        return self

    def __exit__(self, *a):
        self.h.sorted_piecewise_constant_pdf = self.orig


def g4_neo_noise(tag, n_rays, chunk, n_coarse=128, n_fine=256, gain=1.0, full=False, ulp_trials=0, nv=cases.NV):
    """The reference's OWN rounding noise on the rays of fixture g4_neo_<tag>: the same call evaluated by the
    reference in fp32 and by its fp64 twin (module.double(), fp64 rays / latent; the tri-planes stay fp32 because
    index_grid casts its coordinates with .float(), encoder_tp_fusion_conv.py:128-130).  Stored per ray:
    |ref32 - ref64| (max over channels) for every output of the fixture, plus the fp64 values themselves.
    tests/test_gpu_neo360.py uses it to separate well-conditioned rays (contract: 1e-4 on every one) from rays on
    which the reference disagrees with itself.
    ulp_trials > 0 adds that many fp32 runs of the reference with every MLP weight moved by a random amount within
    +-1 ulp (w (1 + eta), eta ~ U(-2^-24, 2^-24), hash-seeded): what ANY faithful fp32 evaluation of the same network
    (another summation order, fused multiply-adds, a split-fp16 matrix pipe) does to the coarse densities, ~1e-6.
    The fp64 twin samples that sensitivity once per ray; on a chaotic ray (descending-bin inversion,
    neo360/model.py:319-331) one sample can land near zero by luck, so the stored noise is the MAXIMUM over the twin
    and the trials."""
    scene, batch = _neo_inputs(n_rays, nv, full)
    state = synth.nerf_tp_state(0, density_gain=gain)
    per_ray = ("rays_o", "rays_d", "viewdirs")
    keys = ("rgb0", "rgb1", "fg1", "bg1", "fgacc1", "lam1", "depth0", "depth1")
    _ref_tp = ref_nerf_tp
    ref_nerf_tp_nv = lambda st, sc: _ref_tp(st, sc, nv=nv)

    def run(net, b):
        acc = {k: [] for k in keys}
        for i in range(0, n_rays, chunk):
            part = {k: (v[i:i + chunk] if k in per_ray else v) for k, v in b.items()}
            res = net(part, False, False, 0.0, 0.0, out_depth=True)
            acc["rgb0"].append(res[0][0]); acc["depth0"].append(res[0][5])
            acc["rgb1"].append(res[1][0]); acc["fg1"].append(res[1][1]); acc["bg1"].append(res[1][2])
            acc["fgacc1"].append(res[1][3]); acc["lam1"].append(res[1][4]); acc["depth1"].append(res[1][5])
        return {k: torch.cat(v, 0) for k, v in acc.items()}

    net32 = ref_nerf_tp_nv(state, scene)
    net32.num_coarse_samples, net32.num_fine_samples = n_coarse, n_fine
    with _MarginProbe(ref.load("models.neo360.helper")) as probe:
        r32 = run(net32, batch)
    # per forward call the reference resamples inside the sphere first, then outside (neo360/model.py:309-331)
    margin_fg = torch.cat(probe.margins[0::2])
    margin_bg = torch.cat(probe.margins[1::2])
    assert margin_fg.shape == (n_rays,) and margin_bg.shape == (n_rays,)
    cdf_fg, cdf_bg = torch.cat(probe.cdfs[0::2]), torch.cat(probe.cdfs[1::2])
    # round 5: how far the reference's OWN cdf moves between its faithful re-evaluations (fp64 twin, +-1 ulp weight trials), per
    # ray: max_i |cdf_run[i] - cdf_fp32[i]|.  The flip margin the tests use (1e-6) was calibrated on random-init densities; sharp
    # (trained-like) densities move the cdf by more, and a ray is flip-prone when its margin is within reach of THAT displacement
    cdfnoise = {"fg": torch.zeros(n_rays, dtype=torch.float64), "bg": torch.zeros(n_rays, dtype=torch.float64)}

    def note_cdfs(p):
        cdfnoise["fg"] = torch.maximum(cdfnoise["fg"], (torch.cat(p.cdfs[0::2]) - cdf_fg).abs().amax(dim=-1))
        cdfnoise["bg"] = torch.maximum(cdfnoise["bg"], (torch.cat(p.cdfs[1::2]) - cdf_bg).abs().amax(dim=-1))
    del net32
    scene64 = dict(scene)
    scene64["latent"] = scene["latent"].double()
    net64 = ref_nerf_tp_nv(state, scene64).double()
    net64.num_coarse_samples, net64.num_fine_samples = n_coarse, n_fine
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    with _MarginProbe(ref.load("models.neo360.helper")) as p64:
        r64 = run(net64, b64)
    note_cdfs(p64)
    del net64
    per_ray_max = lambda d: (d.amax(dim=-1) if d.dim() == 2 and d.shape[-1] == 3 else d.reshape(n_rays))
    trial_noise = {k: torch.zeros(n_rays, dtype=torch.float64) for k in keys}
    for t in range(ulp_trials):
        st = {}
        for name, w in state.items():
            if name.endswith(".weight"):
                eta = synth.uniform(1000 + t, "ulp/" + name, tuple(w.shape), -2.0 ** -24, 2.0 ** -24)
                st[name] = (w.double() * (1.0 + eta.double())).float()
            else:
                st[name] = w
        net_t = ref_nerf_tp_nv(st, scene)
        net_t.num_coarse_samples, net_t.num_fine_samples = n_coarse, n_fine
        with _MarginProbe(ref.load("models.neo360.helper")) as pt:
            rt = run(net_t, batch)
        note_cdfs(pt)
        del net_t
        for k in keys:
            trial_noise[k] = torch.maximum(trial_noise[k], per_ray_max((r32[k].double() - rt[k].double()).abs()))
        print("ulp trial %d: rgb1 max %.2e, bg1 max %.2e, rays >= 1e-5 on bg1: %d" % (
            t, float(trial_noise["rgb1"].max()), float(trial_noise["bg1"].max()), int((trial_noise["bg1"] >= 1e-5).sum())))
    out = {}
    for k in keys:
        assert r64[k].dtype == torch.float64, (k, r64[k].dtype)
        d = (r32[k].double() - r64[k]).abs()
        out["noise_" + k] = torch.maximum(per_ray_max(d), trial_noise[k]).float()
        if ulp_trials:
            out["noise64_" + k] = per_ray_max(d).float()          # the fp64 twin alone, for the record
        if not full:                      # the full-size fixture stays small: the tests only read the noise arrays
            out["ref64_" + k] = r64[k]
    out["margin_fg1"], out["margin_bg1"] = margin_fg, margin_bg
    out["cdfnoise_fg1"], out["cdfnoise_bg1"] = cdfnoise["fg"].float(), cdfnoise["bg"].float()
    print("cdf self-displacement (twin + trials): bg median %.2e p99 %.2e max %.2e; fg max %.2e" % (
        float(cdfnoise["bg"].median()), float(cdfnoise["bg"].quantile(0.99)), float(cdfnoise["bg"].max()), float(cdfnoise["fg"].max())))
    print("margins: bg < 1e-6 on %d rays, < 1e-7 on %d; fg < 1e-6 on %d" % (
        int((margin_bg < 1e-6).sum()), int((margin_bg < 1e-7).sum()), int((margin_fg < 1e-6).sum())))
    # the fp32 run here must be the committed fixture (same code, same inputs)
    fx = np.load(os.path.join(HERE, "g4_neo_%s.npz" % tag))
    for k in keys:
        out["refit_" + k] = np.float32(np.abs(fx[k] - r32[k].numpy()).max())
    save("g4_neo_%s_noise" % tag, **out)


class _ShiftedQuantiles:
    """While active, the reference's inverse-CDF sampler (neo360/helper.py:174-215) draws its deterministic quantiles
    u = linspace(0, 1 - 2^-32, n) SHIFTED by `delta` (clamped to the same range): every threshold u_j = cdf_i that lies
    within |delta| of a quantile is crossed - in one direction - exactly as an fp32 re-evaluation of the coarse level
    with a cdf error of that size and sign would cross it."""

    def __init__(self, helper_module, delta):
        self.h, self.delta = helper_module, float(delta)
        self.orig = helper_module.sorted_piecewise_constant_pdf

    def __enter__(self):
        me = self

        def wrapped(bins, weights, num_samples, randomized, float_min_eps=2 ** -32):
            real = torch.linspace

            def shifted(start, end, steps, **kw):
                return torch.clamp(real(start, end, steps, **kw) + me.delta, float(start), float(end))

            torch.linspace = shifted
            try:
                return me.orig(bins, weights, num_samples, randomized, float_min_eps)
            finally:
                torch.linspace = real

        self.h.sorted_piecewise_constant_pdf = wrapped
        return self

    def __exit__(self, *a):
        self.h.sorted_piecewise_constant_pdf = self.orig


def g4_neo_flip(tag, n_rays, chunk, n_coarse=128, n_fine=256, gain=1.0, full=False, nv=cases.NV, delta=2e-6):
    """PER-RAY size of a sampler flip on the rays of fixture g4_neo_<tag>, measured on the reference itself: its fp32
    forward with the fine-level quantiles shifted by +delta and by -delta (delta = 2 x the flip margin the tests use,
    conftest.FLIP_MARGIN): flip_<k>[ray] = max over the two runs of |shifted - fixture| (max over channels).  On a ray whose
    margin is below the flip margin this is what crossing its near-threshold quantile(s) does to each output; on all
    other rays it is the (tiny) effect of moving 256 samples by 2e-6 of the range.  conftest.check_vs_reference_noise
    bounds a flip-prone ray by ITS OWN flip size instead of the largest one of the fixture."""
    scene, batch = _neo_inputs(n_rays, nv, full)
    state = synth.nerf_tp_state(0, density_gain=gain)
    per_ray = ("rays_o", "rays_d", "viewdirs")
    keys = ("rgb0", "rgb1", "fg1", "bg1", "fgacc1", "lam1", "depth0", "depth1")
    net = ref_nerf_tp(state, scene, nv=nv)
    net.num_coarse_samples, net.num_fine_samples = n_coarse, n_fine

    def run():
        acc = {k: [] for k in keys}
        for i in range(0, n_rays, chunk):
            part = {k: (v[i:i + chunk] if k in per_ray else v) for k, v in batch.items()}
            res = net(part, False, False, 0.0, 0.0, out_depth=True)
            acc["rgb0"].append(res[0][0]); acc["depth0"].append(res[0][5])
            acc["rgb1"].append(res[1][0]); acc["fg1"].append(res[1][1]); acc["bg1"].append(res[1][2])
            acc["fgacc1"].append(res[1][3]); acc["lam1"].append(res[1][4]); acc["depth1"].append(res[1][5])
        return {k: torch.cat(v, 0) for k, v in acc.items()}

    fx = np.load(os.path.join(HERE, "g4_neo_%s.npz" % tag))
    per_ray_max = lambda d: (d.amax(dim=-1) if d.dim() == 2 and d.shape[-1] == 3 else d.reshape(n_rays))
    out = {"flip_" + k: torch.zeros(n_rays, dtype=torch.float64) for k in keys}
    helper = ref.load("models.neo360.helper")
    for d in (delta, -delta):
        with _ShiftedQuantiles(helper, d):
            r = run()
        for k in keys:
            out["flip_" + k] = torch.maximum(out["flip_" + k], per_ray_max((r[k].double() - torch.from_numpy(fx[k]).double()).abs()))
    out = {k: v.float() for k, v in out.items()}
    out["delta"] = np.float64(delta)
    print("flip sizes (%s): bg1 max %.2e, rays with bg1 flip >= 1e-5: %d; rgb1 max %.2e" % (
        tag, float(out["flip_bg1"].max()), int((out["flip_bg1"] >= 1e-5).sum()), float(out["flip_rgb1"].max())))
    save("g4_neo_%s_flip" % tag, **out)


# ---------------------------------------------------------------------------------
# G8 training-side call: NeRF_TP.forward(out_depth=False) deterministic / white background / randomized
# ---------------------------------------------------------------------------------

class _QueuedRand:
    """Stands in for torch.rand while the reference runs randomized=True: hands out prepared uniform tensors in call
    order (helper.py:49 fg, :49 bg, :196 fg, :196 bg), so that the same draws can be given to the oracle and the GPU."""

    def __init__(self, tensors):
        self.queue = list(tensors)

    def __call__(self, *shape, **kw):
        t = self.queue.pop(0)
        shape = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else tuple(shape)
        assert tuple(t.shape) == shape, (t.shape, shape)
        return t


def g8_training(n_rays=64, n_coarse=16, n_fine=24, seed=1234):
    from oracle import training as otrain
    scene = cases.small_scene()
    net = ref_nerf_tp(synth.nerf_tp_state(0), scene)
    net.num_coarse_samples, net.num_fine_samples = n_coarse, n_fine
    batch = cases.neo_batch(cases.strided_rays(n_rays))
    names = ("rgb", "fg_w", "bg_w", "fg_sd", "bg_sd", "bg_acc")
    out = {}
    for tag, randomized, white in (("det", False, False), ("white", False, True), ("rand", True, False)):
        real_rand = torch.rand
        if randomized:
            u = [otrain.philox_uniform(seed, 0, n_rays, n_coarse + 1), otrain.philox_uniform(seed, 1, n_rays, n_coarse + 1),
                 otrain.philox_uniform(seed, 2, n_rays, n_fine), otrain.philox_uniform(seed, 3, n_rays, n_fine)]
            torch.rand = _QueuedRand(u)
        try:
            res = net(batch, randomized, white, 0.0, 0.0, out_depth=False)
        finally:
            torch.rand = real_rand
        for lv in (0, 1):
            for nm, v in zip(names, res[lv]):
                out["%s_%s%d" % (tag, nm, lv)] = v
    # stand-alone stratified sampler and randomized pdf sampler of the reference on the same draws
    HN = ref.load("models.neo360.helper")
    rays = cases.strided_rays(n_rays)
    far = HN.intersect_sphere(rays["rays_o"], rays["rays_d"])
    near = torch.full((n_rays, 1), 1e-4)
    u0, u1 = otrain.philox_uniform(seed, 0, n_rays, n_coarse + 1), otrain.philox_uniform(seed, 1, n_rays, n_coarse + 1)
    real_rand = torch.rand
    torch.rand = _QueuedRand([u0, u1])
    try:
        t_fg, _ = HN.sample_along_rays(rays["rays_o"], rays["rays_d"], n_coarse, near, far, True, False, True)
        s_bg, _, _ = HN.sample_along_rays(rays["rays_o"], rays["rays_d"], n_coarse, near, far, True, False, False, far_uncontracted=3)
    finally:
        torch.rand = real_rand
    out.update(strat_fg=t_fg, strat_bg=s_bg)
    pc = cases.pdf_cases()
    up = otrain.philox_uniform(seed, 7, pc["asc"][0].shape[0], 48)
    for tag in ("asc", "desc"):
        torch.rand = _QueuedRand([up])
        try:
            out["pdf_rand_" + tag] = HN.sorted_piecewise_constant_pdf(pc[tag][0], pc[tag][1], 48, True)
        finally:
            torch.rand = real_rand
    save("g8_training", **out)


# ---------------------------------------------------------------------------------
# G6 Mip-NeRF 360 (models/mipnerf360)
# ---------------------------------------------------------------------------------

def g6_mip360():
    M = ref.load("models.mipnerf360.model")
    H = ref.load("models.mipnerf360.helper")
    out = {"basis": H.generate_basis("icosahedron", 2)}
    rays = cases.mip_rays(160)
    for tag, tf, gain, (n_prop, n_nerf) in (("a", 1.0, 1.0, (64, 32)), ("b", 0.3, 1.0, (64, 32)),
                                             ("sharp", 1.0, 6.0, (64, 32)), ("c", 1.0, 1.0, (64, 128))):
        net = M.MipNeRF360(num_prop_samples=n_prop, num_nerf_samples=n_nerf)
        net.load_state_dict(synth.mip360_state(0, density_gain=gain, weight_gain=0.5), strict=True)
        with torch.enable_grad():
            rend, hist = net(rays, tf, False, False, 0.2, 3.0)
        for lv in range(3):
            out["rgb%d_%s" % (lv, tag)] = rend[lv]["rgb"].detach()
            out["sdist%d_%s" % (lv, tag)] = hist[lv]["sdist"].detach()
            out["w%d_%s" % (lv, tag)] = hist[lv]["weights"].detach()
            out["dens%d_%s" % (lv, tag)] = hist[lv]["density"].detach()
        out["prgb2_%s" % tag] = hist[2]["rgb"].detach()
    # stage fixtures: contraction (incl. the autograd Jacobian), lifting, IPE, dilation, interval sampling
    means = synth.uniform(51, "mip_mean", (40, 7, 3), -2.5, 2.5)
    means[0] *= 0.2                                       # inside the unit ball
    A = synth.uniform(51, "mip_cov", (40, 7, 3, 3), -0.05, 0.05)
    covs = A @ A.transpose(-1, -2)
    with torch.enable_grad():
        cm, cc = H.contract(means, covs, is_train=False)
    lm, lv_ = H.lift_and_diagonalize(cm, cc, out["basis"])
    out.update(con_mean=cm, con_cov=cc, lift_mean=lm, lift_var=lv_, ipe=H.integrated_pos_enc(lm, lv_, 0, 12))
    t = torch.sort(synth.uniform(53, "mip_t", (24, 33), 0.0, 1.0), dim=-1).values
    w = synth.uniform(53, "mip_w", (24, 32), 0.0, 1.0)
    w[1] = 0.0
    w[1, 5] = 1.0
    td, wd = H.max_dilate_weights(t, w, 0.01, domain=(0.0, 1.0), renormalize=True)
    out.update(dil_t=td, dil_w=wd)
    logits = torch.where(td[..., 2:-1] > td[..., 1:-2], torch.log(wd[..., 1:-1]), torch.full_like(wd[..., 1:-1], -torch.inf))
    out["intervals"] = H.sample_intervals(False, td[..., 1:-1], logits, 32, single_jitter=True, domain=(0.0, 1.0))
    save("g6_mip360", **out)


# ---------------------------------------------------------------------------------
# G7 PixelNeRF baseline decoder (models/vanilla_nerf/model_pixel.py)
# ---------------------------------------------------------------------------------

def ref_pixelnerf(state, scene, nv=cases.NV):
    M = ref.load("models.vanilla_nerf.model_pixel")
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        net = M.PixelNeRF(num_src_views=nv)
    enc = net.encoder                       # the reference's SpatialEncoder; only its CNN forward is replaced
    enc.forward = lambda imgs: None         # the image encoder is outside the hot path: latent preset below
    enc.latent = scene["latent"]
    Hf, Wf = scene["latent"].shape[-2:]
    ls = torch.tensor([float(Wf), float(Hf)])
    enc.latent_scaling = ls / (ls - 1) * 2.0
    enc.latent_size = 512
    missing = net.load_state_dict(state, strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("encoder")], missing
    assert not missing.unexpected_keys, missing
    return net.eval()


def g7_pixelnerf():
    scene = cases.small_scene()
    per_ray = ("rays_o", "rays_d", "viewdirs")
    out = {}
    for tag, n_rays, chunk, gain, white in (("a", 300, 256, 1.0, False), ("sharp", 128, 128, 8.0, False),
                                             ("white", 96, 96, 1.0, True)):
        net = ref_pixelnerf(synth.pixelnerf_state(0, density_gain=gain), scene)
        batch = cases.neo_batch(cases.strided_rays(n_rays))
        acc = {k: [] for k in ("rgb0", "acc0", "depth0", "rgb1", "acc1", "depth1")}
        for i in range(0, n_rays, chunk):
            part = {k: (v[i:i + chunk] if k in per_ray else v) for k, v in batch.items()}
            res = net(part, False, white, 0.2, 2.5)
            for lv in (0, 1):
                acc["rgb%d" % lv].append(res[lv][0]); acc["acc%d" % lv].append(res[lv][1]); acc["depth%d" % lv].append(res[lv][2])
        out.update({"%s_%s" % (k, tag): torch.cat(v, 0) for k, v in acc.items()})
    save("g7_pixelnerf", **out)


# ---------------------------------------------------------------------------------
# G9 pillar stage of the scene encoder: GridEncoder.forward from the world grid to the three floor-plans
# ---------------------------------------------------------------------------------

PILLAR_GRID = (12, 10, 8)


def g9_pillar():
    ENC = ref.load("models.neo360.encoder_tp_fusion_conv")
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        enc = ENC.GridEncoder(grid_size=list(PILLAR_GRID))
    missing = enc.load_state_dict(synth.pillar_state(0), strict=False)
    assert not missing.unexpected_keys, missing
    enc.eval()
    scene = cases.small_scene()
    latent = scene["latent"]
    Hf, Wf = latent.shape[-2:]
    ls = torch.tensor([float(Wf), float(Hf)])
    sp = enc.spatial_encoder
    sp.forward = lambda images: None                     # the ResNet is outside the hot path: latent preset
    sp.latent = latent
    sp.latent_scaling = ls / (ls - 1) * 2.0
    captured = {}
    for ax in ("yz", "xz", "xy"):
        getattr(enc, "floorplan_convnet_" + ax).register_forward_pre_hook(
            lambda mod, inp, ax=ax: captured.__setitem__(ax, inp[0].detach().clone()))
    poses, focal, centre = synth.source_views(cases.NV, *cases.IMG_WH)
    images = torch.zeros(cases.NV, 3, cases.IMG_WH[1], cases.IMG_WH[0])
    real_tensor = torch.tensor
    torch.tensor = lambda *a, **k: real_tensor(*a, **{kk: vv for kk, vv in k.items() if kk != "device"})   # :465 hard-codes "cuda"
    try:
        enc(images, poses, focal, centre)
    finally:
        torch.tensor = real_tensor
    # the conv nets receive NCHW permutes of the floor-plans (:580-592).  Stored channels-last, every 4th channel plus
    # the per-cell sum and sum of squares over all 512 channels (keeps the fixture small, still touches every channel)
    out = {}
    for ax in captured:
        fp = captured[ax].permute(0, 2, 3, 1).contiguous()
        out["fp_" + ax] = fp[..., ::4].contiguous()
        out["sum_" + ax] = fp.double().sum(-1)
        out["sq_" + ax] = (fp.double() ** 2).sum(-1)
    save("g9_pillar", **out)


# ---------------------------------------------------------------------------------
# G10 the reference's outputs for the calls of tests/test_oracle_vs_reference.py (same inputs, same seeds)
# ---------------------------------------------------------------------------------

def _quiet(fn, *a, **k):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def g10_live():
    out = {}
    # vanilla NeRF, 64 rays
    net = _quiet(ref.load("models.vanilla_nerf.model").NeRF)
    net.load_state_dict(synth.vanilla_state(0))
    want = net.eval()(cases.strided_rays(64), False, False, 0.2, 3.0)
    out.update(van_rgb0=want[0][0], van_rgb1=want[1][0], van_depth1=want[1][2])
    # PixelNeRF late-fusion MLP stage on synthetic encodings / latents
    M = ref.load("models.vanilla_nerf.model_pixel")
    for nv in (1, 3):
        mlp = _quiet(M.NeRFMLP, 0, 10, 4)
        mlp.load_state_dict(synth.pixelnerf_mlp_state(61 + nv, ""))
        P = 40
        x = synth.uniform(63, "pix_x%d" % nv, (nv, P, 63), -1, 1)
        cond = synth.uniform(63, "pix_c%d" % nv, (nv * P, 27), -1, 1)
        latent = synth.normal(63, "pix_l%d" % nv, (nv * P, 512), 0.3)
        r, s = mlp.eval()(x, cond, latent, combine_inner_dims=(nv, P))
        out["pixmlp_rgb_nv%d" % nv], out["pixmlp_sigma_nv%d" % nv] = r.reshape(-1, 3), s.reshape(-1, 1)
    # PixelNeRF and NeO-360 decoders on the small scene
    scene = cases.small_scene()
    net = ref_pixelnerf(synth.pixelnerf_state(0), scene)
    want = net(cases.neo_batch(cases.strided_rays(48)), False, False, 0.2, 2.5)
    out.update(pix_rgb0=want[0][0], pix_rgb1=want[1][0], pix_depth1=want[1][2])
    net = ref_nerf_tp(synth.nerf_tp_state(0), scene)
    net.num_coarse_samples, net.num_fine_samples = 24, 40
    want = net(cases.neo_batch(cases.strided_rays(40)), False, False, 0.0, 0.0, out_depth=True)
    out.update(neo_rgb0=want[0][0], neo_rgb1=want[1][0], neo_out4_1=want[1][4], neo_out5_1=want[1][5])
    # Mip-NeRF 360, deterministic forward
    M = ref.load("models.mipnerf360.model")
    net = M.MipNeRF360(num_prop_samples=32, num_nerf_samples=16)
    net.load_state_dict(synth.mip360_state(0, weight_gain=0.5), strict=True)
    with torch.enable_grad():
        rend, hist = net(cases.mip_rays(24), 1.0, False, False, 0.2, 3.0)
    out.update(mip_rgb=rend[-1]["rgb"].detach(), mip_sdist=hist[-1]["sdist"].detach())
    # Mip-NeRF 360, randomized forward + autograd gradients of every parameter.  All 9.3 M gradient entries follow from what crossed
    # each MLP's boundary - its input features and the gradients arriving at its heads (cases.mip_mlp_param_grads) - so that is what
    # is stored; the gradients rebuilt from it are checked here against the reference's own autograd result
    n_prop, n_nerf, B = 16, 8, 12
    state = synth.mip360_state(0, weight_gain=0.25)
    net = M.MipNeRF360(num_prop_samples=n_prop, num_nerf_samples=n_nerf)
    net.load_state_dict(state, strict=True)
    seen = {}
    for mname, mod in net.named_modules():
        if isinstance(mod, torch.nn.Linear):
            def fwd(m, inp, res, mname=mname):
                e = seen.setdefault(mname, {"x": [], "dy": []})
                e["x"].append(inp[0].detach().reshape(-1, m.in_features))
                call = len(e["x"]) - 1
                res.register_hook(lambda g, call=call: e["dy"].append((call, g.detach().reshape(-1, m.out_features))))
            mod.register_forward_hook(fwd)
    torch.manual_seed(5)
    with torch.enable_grad():
        rend, hist = net(cases.mip_rays(B), 0.5, True, True, 0.2, 3.0)
        loss_ref = (rend[-1]["rgb"] ** 2).mean() + sum((h["weights"] ** 2).sum(-1).mean() for h in hist)
        names = [k for k, p in net.named_parameters()]
        g_ref = torch.autograd.grad(loss_ref, [p for _, p in net.named_parameters()], allow_unused=True)
    for lvl in range(3):
        out["rnd_sdist%d" % lvl] = hist[lvl]["sdist"].detach()
        out["rnd_w%d" % lvl] = hist[lvl]["weights"].detach()
    out["rnd_rgb"] = rend[-1]["rgb"].detach()
    out["rnd_names"] = np.frombuffer("\n".join(names).encode(), dtype=np.uint8)       # parameter order, as bytes (fixtures load as tensors)
    out["rnd_unused"] = np.array([g is None for g in g_ref])
    xs = lambda name: torch.cat(seen[name]["x"])
    dys = lambda name: torch.cat([g for _, g in sorted(seen[name]["dy"], key=lambda c: c[0])])
    rebuilt = {}
    for m in sorted({k.split(".pts_linear")[0] for k in names if ".pts_linear" in k}):
        tag = m.replace(".", "")
        out["rnd_x0_" + tag], out["rnd_dyd_" + tag] = xs(m + ".pts_linear.0"), dys(m + ".density_layer")
        if m + ".rgb_layer" in seen:
            width = net.get_submodule(m + ".bottleneck_layer").out_features
            out["rnd_dir_" + tag], out["rnd_dyrgb_" + tag] = xs(m + ".views_linear.0")[:, width:], dys(m + ".rgb_layer")
        rebuilt.update(cases.mip_mlp_param_grads(state, m + ".", out["rnd_x0_" + tag], out["rnd_dyd_" + tag],
                                                 out.get("rnd_dir_" + tag), out.get("rnd_dyrgb_" + tag)))
    for k, g in zip(names, g_ref):
        if g is not None:
            assert float((rebuilt[k] - g).norm()) <= 1e-5 * float(g.norm()) + 1e-12, (k, float((rebuilt[k] - g).norm() / g.norm()))
    save("g10_live", **out)


def main(which):
    jobs = {
        "g1": g1_raygen, "g2": g2_aabb, "g3": g3_stages, "g3n": g3_pdf_noise, "g4v": g4_vanilla,
        # small: what the CPU oracle test re-runs; two chunks (256 + 44): quirk Q1 + short last chunk
        "g4n_small": lambda: g4_neo("small", 300, 256, 32, 64),
        # G5 chunk-dependence regression: same rays, chunk 128 vs 64
        "g5a": lambda: g4_neo("c128", 128, 128, 32, 64),
        "g5b": lambda: g4_neo("c64", 128, 64, 32, 64),
        # reference-default sample counts: one 1024-ray chunk and a 1500-ray two-chunk case (GPU tests)
        "g4n_1024": lambda: g4_neo("1024", 1024, 1024),
        "g4n_1500": lambda: g4_neo("1500", 1500, 1024),
        "g4n_sharp": lambda: g4_neo("sharp", 256, 256, 32, 64, gain=8.0),
        # other source-view counts (the reference builds NeRF_TP(num_src_views=int(render_name[0])), model.py:606-616)
        "g4n_nv1": lambda: g4_neo("nv1", 96, 96, 32, 64, nv=1),
        "g4n_nv2": lambda: g4_neo("nv2", 96, 96, 32, 64, nv=2),
        "g4n_nv5": lambda: g4_neo("nv5", 96, 96, 32, 64, nv=5),
        # the reference's own fp32-vs-fp64 disagreement on the same rays (conditioning of the fine-level resampling)
        "g4n_1024_noise": lambda: g4_neo_noise("1024", 1024, 1024),
        "g4n_1500_noise": lambda: g4_neo_noise("1500", 1500, 1024),
        "g4n_sharp_noise": lambda: g4_neo_noise("sharp", 256, 256, 32, 64, gain=8.0),
        # BASELINE C3 at FULL size: one reference chunk (1024 rays of the 640x480 bench frame), tri-planes 3x128x120x160,
        # latents 3x512x240x320, 128 + 256 samples (neo360/model.py:266-581, :169-171; chunk 1024: opt.py:195-200),
        # and the reference's fp64 twin on the same rays.  ~10 GB of RAM, a few minutes.
        "g4n_full": lambda: g4_neo("full", 1024, 1024, full=True),
        "g4n_full_noise": lambda: g4_neo_noise("full", 1024, 1024, full=True, ulp_trials=2),
        # four more full-size chunks (cases.FULL_B): another strip, two other target poses, five source views; each with
        # its fp64 twin, two +-1 ulp trials and the cdf margins (VERDICT r3 task 6)
        # round 5: b5 (density gain 8: trained-like) and b6 (second feature seed, std 0.5) - cases.FULL_B
        **{"g4n_full_%s" % t: (lambda t=t: g4_neo("full_" + t, 1024, 1024, full=t, nv=cases.FULL_B[t]["nv"], gain=cases.full_gain(t)))
           for t in cases.FULL_B},
        **{"g4n_full_%s_noise" % t: (lambda t=t: g4_neo_noise("full_" + t, 1024, 1024, full=t, ulp_trials=2, nv=cases.FULL_B[t]["nv"],
                                                              gain=cases.full_gain(t))) for t in cases.FULL_B},
        # per-ray flip sizes (quantiles shifted by +-2e-6 inside the reference's sampler) for every fixture that has a noise twin
        "g4n_1024_flip": lambda: g4_neo_flip("1024", 1024, 1024),
        "g4n_1500_flip": lambda: g4_neo_flip("1500", 1500, 1024),
        "g4n_sharp_flip": lambda: g4_neo_flip("sharp", 256, 256, 32, 64, gain=8.0),
        "g4n_full_flip": lambda: g4_neo_flip("full", 1024, 1024, full=True),
        **{"g4n_full_%s_flip" % t: (lambda t=t: g4_neo_flip("full_" + t, 1024, 1024, full=t, nv=cases.FULL_B[t]["nv"],
                                                            gain=cases.full_gain(t))) for t in cases.FULL_B},
        "g6": g6_mip360,
        "g7": g7_pixelnerf,
        "g8": g8_training,
        "g9": g9_pillar,
        "g10": g10_live,
    }
    for name, fn in jobs.items():
        if not which or name in which:
            fn()


if __name__ == "__main__":
    if not ref.reference_available():
        sys.exit("reference tree not found at %s" % ref.REFERENCE_ROOT)
    main(set(sys.argv[1:]))
