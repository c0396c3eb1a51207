"""Case table of the scene axis of the inference path: source-view counts 1..8 and feature-map sizes from the API minimum (2 x 2)
over maps that leave a tail in the 64-texel groups of the pre-projection up to the small scene of every other test.  Plain CPU
torch: tests/test_view_map_cases_cpu.py checks the conditions of every case (finite fp64 references, the fp32 oracle inside half
of every bound, every map a kernel reads really read) on the very inputs tests/test_gpu_view_map_sweep.py hands to the kernels.

Scenes: (NV; plane H x W; latent H x W), SCENES below.  Texels per map (NV H W): 4 / 4, 30 / 70, 90 / 210, 48 / 48, 45 / 105 - tails
below and above one 64-texel group - and the multiples of 64 of the small scene.  Views 1..5 are synth.source_views(5) bit for bit,
views 6..8 three further synth.look_at_origin poses.

Point shapes (R rays, N samples, chunk): P = R N = 1, 63, 64, 65, 129 and 203 (no multiple of 32); chunk 4 of 9 rays and 2 of 3
rays do not divide R, chunk 16 of 8 rays exceeds it.  The view-direction tiling (quirk Q1) makes the colours depend on the chunk,
so the oracle is evaluated per chunk slice.  Shapes rotate over the scenes (CASES): every scene meets P = 64 and a P = 1 (mod 64),
the two NV = 8 scenes meet every shape between them.

Sample rows: inside the sphere linspace(0.03, 0.97, N) x far; outside descending inverse radii BG_S_HI .. BG_S_LO, concentrated
towards s -> 0 so that the looked-up points o + (far (1 - s) + 3 s) d stay near the sphere, on the planes and in front of the cameras.

Bounds (per entry): constant x max(1, largest |fp64 value| of that output in the case), the constants being those of the
single-scene tests: EVAL = 2e-5 for evaluator rgb and sigma (test_gpu_neo360_stages.py, test_gpu_pixelnerf.py), PLAN = 2e-5 for
floor-plans (test_gpu_encoder.py), alongray_cases.LOOKUP = 1e-5 for lookups.  Variant agreement: AGREE_RGB / AGREE_SIGMA of
test_preprojection_is_a_reassociation.
"""
import functools
import math

import torch

import cases
import oracle
from alongray_cases import LOOKUP, scale_of, worst_entry
from neo360_amd import synth

EVAL = 2e-5
PLAN = 2e-5
AGREE_RGB, AGREE_SIGMA = 5e-6, 2e-5
MIN_READ_FRACTION, MIN_READ_PAIRS = 0.10, 8      # of the (point, view) pairs of a case, per map the kernel reads

MAX_VIEWS = 8
EXTRA_VIEWS = ((170.0, 0.45, 0.5), (265.0, 0.75, 0.15), (335.0, 0.55, -0.2))      # views 6..8: azimuth, radius, height

SMALL = (cases.PLANE_HW, cases.LATENT_HW)
# (NV, plane H x W, latent H x W)
SCENES = ((1, (2, 2), (2, 2)),            # 0: the API minimum, 4 texels
          (2, (3, 5), (5, 7)),            # 1: 30 and 70 texels
          (4,) + SMALL,                   # 2
          (6, (3, 5), (5, 7)),            # 3: 90 and 210 texels
          (7,) + SMALL,                   # 4: inexact 1 / NV
          (8, (2, 3), (3, 2)),            # 5: the limit on tiny maps, 48 texels
          (8,) + SMALL,                   # 6
          (3, (3, 5), (5, 7)))            # 7: the anchor view count on odd maps, 45 and 105 texels
# (R, N, chunk)
SHAPES = {1: (1, 1, 1), 63: (9, 7, 4), 64: (8, 8, 16), 65: (5, 13, 5), 129: (3, 43, 2), 203: (7, 29, 7)}
ROTATION = ((64, 1, 203), (64, 65, 63), (64, 129, 203), (64, 1, 63), (64, 65, 203), (64, 1, 63, 203), (64, 65, 129), (64, 129, 63))
CASES = tuple((s, p) for s, ps in enumerate(ROTATION) for p in ps)                # (scene index, P)

# target pose of the rays (cases.crop_rays: azimuth, radius, height) and the inverse-radius range outside the sphere.  The one ray of
# a P = 1 case starts next to the origin, where every source camera looks: from the test orbit its only point lies outside most
# source frusta and the case would read no latent texel at all.
TARGET = dict(azimuth=40.0, radius=0.6, height=0.3)
TARGET_ONE_POINT = dict(azimuth=10.0, radius=0.05, height=0.02)      # faces view 1 (azimuth 0): its point outside the sphere is in that frustum
BG_S_HI, BG_S_LO = 0.35, 0.01

NEO_VARIANTS = ("f16x3", "f16x3-pp1", "f16x3-pp2", "f16x3-noproj", "f32", "f32-pp1", "f32-noproj")
PIX_VARIANTS = (("f16x3", True), ("f16x3", False), ("f32", True), ("f32", False))
FG_SLOT, FG_PREFIX = 0, "fg_coarse_mlp."
BG_SLOT, BG_PREFIX = 3, "bg_fine_mlp."
PIX_SLOT, PIX_PREFIX = 1, "fine_mlp."

# fused render: scene index, (coarse, fine) sample counts, rays
RENDER_SCENES = (0, 5, 6)
RENDER_SAMPLES = (16, 24)
RENDER_RAYS = 48
CULL_EPS = 1e-2
# foreground density bias that makes a mixed frame at CULL_EPS (the trick of test_gpu_cull_background.py); on the CPU oracle the
# culled fractions are 0.56, 0.63 and 0.42 (tests/test_view_map_cases_cpu.py keeps them inside 0.3 .. 0.7)
CULL_BIAS = {0: 4.0, 5: 3.9, 6: 3.9}

# pillar stage: (NV, latent H x W, grid); M = NV G0 G1 G2 = 1, 63, 64, 65, 378 (tail 58), 315, 840, 512 (the axis limit)
PILLAR = ((1, (2, 2), (1, 1, 1)), (1, (5, 7), (3, 7, 3)), (8, (3, 2), (2, 4, 1)), (5, (5, 7), (13, 1, 1)),
          (6, (5, 7), (3, 7, 3)), (7, cases.LATENT_HW, (5, 3, 3)), (8, cases.LATENT_HW, (5, 7, 3)), (2, cases.LATENT_HW, (256, 1, 1)))
PILLAR_GRAD = (0, 2, 3, 4)               # of PILLAR: M = 1, NV = 8 (M = 64), M = 65, M = 378
PILLAR_PARAM_SEED = 2

# training lookups: scene index -> all scatter traffic lands on 4 (scenes 0, 5 have 2 x 2 / 3 x 2 latents) or 35 texels per view
LOOKUP_SCENES = ((2, (2, 2), (2, 2)), (8, (2, 2), (2, 2)), (2, (3, 5), (5, 7)), (8, (3, 5), (5, 7)))
LOOKUP_RAYS, LOOKUP_SAMPLES = 5, 13      # P = 65 ray-ordered points


def _d(x):
    return x.detach()


def views(nv, W=cases.IMG_WH[0], H=cases.IMG_WH[1]):
    """poses (nv,4,4), focal (nv,), centre (nv,2) of nv = 1..8 source views: the first five are synth.source_views(5) bit for bit."""
    assert 1 <= nv <= MAX_VIEWS
    poses, focal, centre = synth.source_views(min(nv, 5), W, H)
    if nv > 5:
        more = torch.stack([synth.look_at_origin(*EXTRA_VIEWS[i]) for i in range(nv - 5)])
        poses = torch.cat([poses, more])
        focal = torch.full((nv,), 0.8 * W)
        centre = torch.tensor([[W / 2.0, H / 2.0]]).repeat(nv, 1)
    return poses, focal, centre


@functools.lru_cache(maxsize=None)
def scene(nv, plane_hw, latent_hw, seed=7):
    sc = synth.scene_features(seed, nv, 128, tuple(plane_hw), 512, tuple(latent_hw), std=0.5)
    sc["image_wh"] = (float(cases.IMG_WH[0]), float(cases.IMG_WH[1]))
    return sc


def scene_of(s):
    nv, plane_hw, latent_hw = SCENES[s]
    return scene(nv, plane_hw, latent_hw, 7 + s)


def batch(rays, nv):
    poses, focal, centre = views(nv)
    out = dict(rays)
    out.update(src_poses=poses, src_focal=focal, src_c=centre, src_imgs=torch.zeros(nv, 3, cases.IMG_WH[1], cases.IMG_WH[0]))
    return out


PER_RAY = ("rays_o", "rays_d", "viewdirs")


def chunk_of(b, i, chunk):
    return {k: (v[i:i + chunk] if k in PER_RAY else v) for k, v in b.items()}


def to64(x):
    if isinstance(x, dict):
        return {k: to64(v) for k, v in x.items()}
    return x.double() if isinstance(x, torch.Tensor) and x.is_floating_point() else x


@functools.lru_cache(maxsize=None)
def point_case(s, P):
    """Inputs of one (scene, shape) case: batch (R rays of the scene's target pose + its source views), far (R,1), the sample rows
    inside (t, ascending) and outside (inverse radius, descending) the sphere, the chunk."""
    R, N, chunk = SHAPES[P]
    nv = SCENES[s][0]
    b = batch(cases.strided_rays(R, **(TARGET_ONE_POINT if P == 1 else TARGET)), nv)
    far, hit = oracle.rays.sphere_exit_depth(b["rays_o"], b["rays_d"])
    t_in = (torch.linspace(0.03, 0.97, N)[None, :] * far).contiguous()
    s_out = torch.linspace(BG_S_HI, BG_S_LO, N)[None, :].repeat(R, 1).contiguous()
    return dict(batch=b, far=far, hit=hit, t_in=t_in, s_out=s_out, chunk=chunk, R=R, N=N, nv=nv)


def _per_chunk(fn, c, tv, dtype):
    """fn(batch slice, tvals slice, far slice) per chunk slice of the case, concatenated: (R,N,4) = rgb | sigma."""
    cast = to64 if dtype == torch.float64 else (lambda x: x)
    out = []
    for i in range(0, c["R"], c["chunk"]):
        rgb, sigma = fn(cast(chunk_of(c["batch"], i, c["chunk"])), cast(tv[i:i + c["chunk"]]), cast(c["far"][i:i + c["chunk"]]))
        out.append(torch.cat([rgb, sigma], dim=-1))
    return _d(torch.cat(out))


def _cast_params(params, dtype):
    return {k: v.to(dtype) for k, v in params.items()}


@functools.lru_cache(maxsize=None)
def _neo_params(dtype):
    return _cast_params(synth.nerf_tp_state(0), dtype)


@functools.lru_cache(maxsize=None)
def _pix_params(dtype):
    return _cast_params(synth.pixelnerf_state(0), dtype)


def _scene_cast(sc, dtype):
    return {k: (v.to(dtype) if isinstance(v, torch.Tensor) else v) for k, v in sc.items()}


def neo_eval(s, P, params, sc, dtype):
    """(inside, outside) per-point outputs (R,N,4) of oracle.neo360.region_eval on case (s, P) with the state dict `params` and the
    scene `sc`, both cast to `dtype`, per chunk slice."""
    c, sc, p = point_case(s, P), _scene_cast(sc, dtype), _cast_params(params, dtype)
    fg = _per_chunk(lambda b, tv, far: oracle.neo360.region_eval(p, FG_PREFIX, b, sc, tv, True, far), c, c["t_in"], dtype)
    bg = _per_chunk(lambda b, tv, far: oracle.neo360.region_eval(p, BG_PREFIX, b, sc, tv, False, far), c, c["s_out"], dtype)
    return fg, bg


@functools.lru_cache(maxsize=None)
def neo_reference(s, P, dtype=torch.float64):
    """(inside, outside) per-point outputs (R,N,4) of oracle.neo360.region_eval in `dtype`, per chunk slice."""
    return neo_eval(s, P, _neo_params(dtype), scene_of(s), dtype)


def pix_eval(s, P, params, sc, dtype):
    """Per-point outputs (R,N,4) of oracle.pixelnerf.region_eval on case (s, P) with `params` and `sc`, cast to `dtype`."""
    c, sc, p = point_case(s, P), _scene_cast(sc, dtype), _cast_params(params, dtype)
    return _per_chunk(lambda b, tv, far: oracle.pixelnerf.region_eval(p, PIX_PREFIX, b, sc, tv), c, c["t_in"], dtype)


@functools.lru_cache(maxsize=None)
def pix_reference(s, P, dtype=torch.float64):
    return pix_eval(s, P, _pix_params(dtype), scene_of(s), dtype)


def eval_checks(got, ref64, ref32):
    """got (R,N,4) of an evaluator -> {rgb, sigma: worst_entry} under EVAL x max(1, largest |fp64 value| of that output)."""
    got = torch.as_tensor(got).detach().cpu()
    return dict(rgb=worst_entry(got[..., :3], ref64[..., :3], EVAL * scale_of(ref64[..., :3]), ref32[..., :3]),
                sigma=worst_entry(got[..., 3:], ref64[..., 3:], EVAL * scale_of(ref64[..., 3:]), ref32[..., 3:]))


# ---- which maps a case really reads (fp64 coordinates) ----------------------------------------------------------------------------
def _tap_weight_nonzero(g, H, W):
    """g (...,2) grid coordinates (x -> W, y -> H), align_corners=True, zero padding: True where at least one of the four taps lies on
    the map with a non-zero weight."""
    x = (g[..., 0] + 1) / 2 * (W - 1)
    y = (g[..., 1] + 1) / 2 * (H - 1)
    x0, y0 = torch.floor(x), torch.floor(y)
    any_tap = torch.zeros(x.shape, dtype=torch.bool)
    for yi, wy in ((y0, y0 + 1 - y), (y0 + 1, y - y0)):
        for xi, wx in ((x0, x0 + 1 - x), (x0 + 1, x - x0)):
            any_tap |= (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1) & (wx * wy != 0)
    return any_tap


def lookup_points(c, inside):
    """World points (R N, 3) in fp64 at which the case's lookups happen."""
    o, d = c["batch"]["rays_o"].double(), c["batch"]["rays_d"].double()
    depth = c["t_in"].double() if inside else c["far"].double() * (1.0 - c["s_out"].double()) + 3.0 * c["s_out"].double()
    return (o[:, None, :] + depth[..., None] * d[:, None, :]).reshape(-1, 3)


def read_fractions(s, P, inside, flip_y=True):
    """{map: (fraction, count) of the (point, view) pairs of the case with a non-zero bilinear weight on that map}."""
    c = point_case(s, P)
    nv, plane_hw, latent_hw = SCENES[s]
    b = c["batch"]
    cam = oracle.gather.world_to_camera(lookup_points(c, inside), b["src_poses"].double())
    f = b["src_focal"][0].double() * torch.tensor([1.0, -1.0 if flip_y else 1.0], dtype=torch.float64)
    uv = oracle.gather.project(cam, f, b["src_c"][0].double())
    g = uv * (oracle.gather.latent_scaling(*latent_hw).double() / torch.tensor(cases.IMG_WH, dtype=torch.float64)) - 1.0
    masks = dict(latent=_tap_weight_nonzero(g, *latent_hw), plane_xz=_tap_weight_nonzero(cam[..., [0, 2]], *plane_hw),
                 plane_xy=_tap_weight_nonzero(cam[..., [0, 1]], *plane_hw), plane_yz=_tap_weight_nonzero(cam[..., [1, 2]], *plane_hw))
    return {k: (float(m.double().mean()), int(m.sum())) for k, m in masks.items()}


def enough_pairs(s, P):
    """The floor of the sensitivity condition for a case: 10 % of its (point, view) pairs and at least 8 pairs.  A P = 1 case has NV
    <= 8 pairs in all, and outside the sphere no point is inside the frusta of eight cameras spread around the orbit: there the floor
    is one pair per map (the case is about the one-row tile, and every scene that has it also has cases under the full floor)."""
    if P == 1:
        return 1
    return max(MIN_READ_PAIRS, math.ceil(MIN_READ_FRACTION * P * SCENES[s][0]))


# ---- pillar stage ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pillar_case(i):
    nv, latent_hw, grid = PILLAR[i]
    sc = scene(nv, (2, 2), latent_hw, 19 + i)
    poses, focal, centre = views(nv)
    return dict(nv=nv, grid=grid, scene=sc, latent=sc["latent"], image_wh=sc["image_wh"], poses=poses, focal=focal, centre=centre,
                params=synth.pillar_state(PILLAR_PARAM_SEED))


def pillar_eval(i, params, latent, dtype):
    """The three floor-plans (yz, xz, xy) of oracle.pillar.floorplans on pillar case i with `params` and `latent`, cast to `dtype`."""
    c = pillar_case(i)
    p = _cast_params(params, dtype)
    out = oracle.pillar.floorplans(p, latent.to(dtype), c["image_wh"], c["poses"].to(dtype), c["focal"].to(dtype),
                                   c["centre"].to(dtype), c["grid"])
    return tuple(_d(x) for x in out)


@functools.lru_cache(maxsize=None)
def pillar_reference(i, dtype=torch.float64):
    """The three floor-plans (yz, xz, xy) of oracle.pillar.floorplans in `dtype`."""
    c = pillar_case(i)
    return pillar_eval(i, c["params"], c["latent"], dtype)


def plan_checks(got, ref64, ref32):
    return {k: worst_entry(g, a, PLAN * scale_of(a), b) for k, g, a, b in zip(("yz", "xz", "xy"), got, ref64, ref32)}


# ---- training lookups --------------------------------------------------------------------------------------------------------------
MAPS = ("plane_xz", "plane_xy", "plane_yz", "latent")


@functools.lru_cache(maxsize=None)
def lookup_case(i):
    """Ray-ordered points (P,3) over a tiny scene, its batch, and the upstream gradients of the looked-up rows."""
    nv, plane_hw, latent_hw = LOOKUP_SCENES[i]
    sc = scene(nv, plane_hw, latent_hw, 31 + i)
    b = batch(cases.strided_rays(LOOKUP_RAYS), nv)
    far, _ = oracle.rays.sphere_exit_depth(b["rays_o"], b["rays_d"])
    t = (torch.linspace(0.05, 0.95, LOOKUP_SAMPLES)[None, :] * far).contiguous()
    pts = oracle.sampling.points_on_rays(t, b["rays_o"], b["rays_d"]).reshape(-1, 3).contiguous()
    gen = torch.Generator().manual_seed(70 + i)
    up = dict(world=torch.randn(nv * pts.shape[0], 128, generator=gen), local=torch.randn(nv * pts.shape[0], 512, generator=gen),
              map=torch.randn(nv * pts.shape[0], 64, generator=gen))
    gmap = torch.randn(nv * latent_hw[0] * latent_hw[1], 64, generator=gen) * 0.5
    return dict(nv=nv, scene=sc, batch=b, pts=pts, up=up, gmap=gmap, latent_hw=latent_hw)


@functools.lru_cache(maxsize=None)
def lookup_reference(i, dtype=torch.float64):
    """world, local, the caller-owned map's rows and the gradients of sum(rows x upstream) with respect to the four scene maps and
    the caller-owned map: autograd of oracle.gather in `dtype`."""
    c = lookup_case(i)
    cv = lambda x: x.to(dtype)
    b, sc, nv = c["batch"], c["scene"], c["nv"]
    Hf, Wf = c["latent_hw"]
    with torch.enable_grad():
        cm = {k: cv(sc[k]).clone().requires_grad_(True) for k in MAPS}
        m = cv(c["gmap"]).clone().requires_grad_(True)
        world = oracle.gather.triplane_features(cv(c["pts"]), cm["plane_xz"], cm["plane_xy"], cm["plane_yz"], cv(b["src_poses"]))
        local = oracle.gather.pixel_aligned_features(cv(c["pts"]), cm["latent"], cv(b["src_poses"]), cv(b["src_focal"]), cv(b["src_c"]),
                                                     sc["image_wh"])
        rows = oracle.gather.pixel_aligned_features(cv(c["pts"]), m.reshape(nv, Hf, Wf, 64).permute(0, 3, 1, 2), cv(b["src_poses"]),
                                                    cv(b["src_focal"]), cv(b["src_c"]), sc["image_wh"])
        loss = (world * cv(c["up"]["world"])).sum() + (local * cv(c["up"]["local"])).sum() + (rows * cv(c["up"]["map"])).sum()
        grads = torch.autograd.grad(loss, [cm[k] for k in MAPS] + [m])
    res = dict(world=_d(world), local=_d(local), map_rows=_d(rows))
    res.update({"g_" + k: g for k, g in zip(MAPS + ("map",), grads)})
    return res


def lookup_checks(got, ref64, ref32):
    return {k: worst_entry(got[k], ref64[k], LOOKUP * scale_of(ref64[k]), ref32[k]) for k in got}


# ---- fused render ------------------------------------------------------------------------------------------------------------------
def render_state(s):
    st = synth.nerf_tp_state(0)
    for k in ("fg_coarse_mlp.density_layer.bias", "fg_fine_mlp.density_layer.bias"):
        st[k] = st[k] + CULL_BIAS[s]
    return st


def render_batch(s):
    return batch(cases.strided_rays(RENDER_RAYS), SCENES[s][0])
