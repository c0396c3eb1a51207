"""Shared inputs and restatements of the vanilla marching-frame tests (tests/test_vanilla_march_cpu.py,
tests/test_gpu_vanilla_march.py; include/neo360_hip.h: VANILLA MARCHING FRAME).  Nothing here depends on the GPU.

Inputs.  synth.vanilla_state(0) with the density-layer bias of both MLPs raised by BIAS[counts], seen by cases.strided_rays(R)
between NEAR and FAR.  BIAS is fixed HERE, on the CPU oracle at eps = EPS: for every count pair whose level 1 is longer than one
segment at least a quarter of the rays stop before N1 and at least a quarter never stop, which tests/test_vanilla_march_cpu.py
asserts - so the GPU tests of the stop rule cannot pass vacuously.  Count pairs (n_coarse, n_fine):

    3 + 4      rows 4 / 8: one short segment, skipping only
    7 + 64     rows 8 / 72 = 64 + 8
    63 + 64    rows 64 / 128: whole segments
    64 + 128   rows 65 / 193: a last segment of ONE sample, the one with the 1e10 interval

    positions / cell_box / keep_rule_box   the BOX KEEP RULE in fp32 - eager torch multiplies and adds separately, like the library
                                           built with -ffp-contract=off - and in fp64 from the same fp32 inputs and fp32 scale;
    near_face_box                          the samples the two may disagree on (see there);
    transmittance0 / stops                 the MODE-0 STOP RULE from the composite's inclusive product;
    oracle_render_marching                 oracle.vanilla.render with the rows of the samples that are not evaluated zeroed before
                                           their composite.
"""
import torch

import cases
import occupancy_cases as oc
import oracle
import terminate_cases as tc
from neo360_amd import synth

# One bias per count pair.  The synthetic MLPs are close to a uniform fog (the boundary transmittances of the 257 rays lie within
# about +-10 % of each other), and where the level-1 boundaries fall in that fog depends on the counts, so no single bias puts eps
# between the rays' boundary transmittances for all pairs at once (at 63 + 64 the 64th of the 128 merged samples is reached after
# about half of the fine samples, whatever the density: only a fog that is opaque within the first coarse interval stops there).
# Each value was found by bisection on the CPU oracle and splits the rays roughly in half; tests/test_vanilla_march_cpu.py asserts
# the quarter / quarter mix for every pair and ray count.  3 + 4 has one segment: nothing can stop.
BIAS = {(3, 4): 5.7, (7, 64): 5.7, (63, 64): 43.7, (64, 128): 2.38}
EPS = 1e-2
NEAR, FAR = 0.2, 3.0
SEGMENT = 64
COUNTS = ((3, 4), (7, 64), (63, 64), (64, 128))
RAYS = (1, 63, 64, 65, 257)
FACE_TOL = 2.0 ** -20           # relative: see near_face_box
# The scene box of the tests: the camera of cases.strided_rays sits at radius 0.6 and looks at the origin, so the samples between
# NEAR and FAR run through this box and out of it on every ray.  SMALL lies inside the span of every ray (clip tests).
BOX = ((-0.9, -0.8, -0.7), (0.8, 0.9, 1.0))
SMALL = ((-0.35, -0.3, -0.3), (0.3, 0.35, 0.4))
FAR_AWAY = ((40.0, 40.0, 40.0), (41.0, 42.0, 43.0))      # holds no sample of any ray


def state(bias):
    """synth.vanilla_state(0) with both density-layer biases raised by `bias` (a number, or a count pair: its entry of BIAS)."""
    if isinstance(bias, tuple):
        bias = BIAS[bias]
    st = synth.vanilla_state(0)
    for k in ("coarse_mlp.density_layer.bias", "fine_mlp.density_layer.bias"):
        st[k] = st[k] + bias
    return st


def rays(n):
    return cases.strided_rays(n)


def n_level(counts):
    return counts[0] + 1, counts[0] + 1 + counts[1]


def box_scale(box, G):
    """scale_a = (float)G / (hi_a - lo_a): one fp32 subtraction and one fp32 division, as the host code of the library."""
    lo = torch.tensor(box[0], dtype=torch.float32)
    hi = torch.tensor(box[1], dtype=torch.float32)
    return lo, torch.tensor(float(G), dtype=torch.float32) / (hi - lo)


def cell_box(x, box, G):
    """floor((x - lo) * scale) per coordinate in x's own dtype (lo and scale are the fp32 values), as a float tensor: no clamp."""
    lo, scale = box_scale(box, G)
    return torch.floor((x - lo.to(x.dtype).to(x.device)) * scale.to(x.dtype).to(x.device))


def keep_rule_box(occ, box, rays_o, dirs, t, clip=False, dtype=torch.float32):
    """(B,N) bool: a coordinate of x is not finite, or occ is None, or x is outside the box and clip is false, or x is inside and
    its cell is set."""
    x = oc.positions(rays_o, dirs, t, dtype)
    wild = ~torch.isfinite(x).all(dim=-1)
    if occ is None:
        return torch.ones_like(wild)
    G = occ.shape[0]
    c = cell_box(x, box, G)
    inside = ((c >= 0) & (c < G)).all(dim=-1)
    ci = torch.where(inside[..., None], c, torch.zeros_like(c)).long()
    bit = occ.to(x.device)[ci[..., 0], ci[..., 1], ci[..., 2]]
    return wild | torch.where(inside, bit, torch.full_like(bit, not clip))


def near_face_box(box, rays_o, dirs, t, G):
    """(B,N) bool: the samples a fp32 and a fp64 statement of the rule may disagree on.  u = (x - lo) scale is formed in fp32 from
    o, t d and lo with four roundings, each relative to its operands, so the fp32 u differs from the fp64 one by less than
    2^-22 (|o| + |t d| + |lo|) scale; a sample is left out when u lies within FACE_TOL = 2^-20 times that magnitude (a factor of
    four above the roundings) of an integer - the cell faces, the faces of the box among them."""
    o, d, tt = (v.double() for v in (rays_o, dirs, t))
    lo, scale = (v.double() for v in box_scale(box, G))
    td = tt[:, :, None] * d[:, None, :]
    x = o[:, None, :] + td
    u = (x - lo) * scale
    mag = (o[:, None, :].abs() + td.abs() + lo.abs()) * scale
    return ((u - torch.round(u)).abs() <= FACE_TOL * mag).any(dim=-1) & torch.isfinite(x).all(dim=-1)


def ball(G, radius=0.55):
    """bool (G,G,G): cells whose centre lies within `radius` half-widths of the box's centre (1.0 touches the faces)."""
    c = (torch.arange(G, dtype=torch.float64) + 0.5) * (2.0 / G) - 1.0
    return c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2 <= radius * radius


def mixed(G):
    """The mixed grid of the tests: a centred ball united with a 3-D checkerboard, so that kept and skipped samples alternate along
    every ray and the compact tiles are ragged."""
    return ball(G) | oc.checkerboard(G)


def transmittance0(sigma, t, rays_d, dtype=torch.float32):
    """(R,N) inclusive product of 1 - alpha + 1e-10 of oracle.compositing.vanilla_composite, in `dtype` from the fp32 inputs:
    delta_i = t_{i+1} - t_i, the last 1e10, times |rays_d|.  Entry b - 1 is the transmittance in front of sample b."""
    sigma, t, d = (v.float().to(dtype) for v in (sigma, t, rays_d))
    delta = torch.cat([t[..., 1:] - t[..., :-1], torch.ones_like(t[..., :1]) * 1e10], dim=-1)
    delta = delta * torch.norm(d[..., None, :], dim=-1)
    alpha = 1.0 - torch.exp(-sigma * delta)
    return torch.cumprod(1.0 - alpha + 1e-10, dim=-1)


stops = tc.stops
near_threshold = tc.near_threshold
zero_behind = tc.zero_behind


def front(stop, N):
    return torch.arange(N, device=stop.device)[None, :] < stop[:, None]


def oracle_render_marching(params, b, counts, eps, occ=None, box=None, clip=False, segment=SEGMENT, coarse=False, white_bkgd=False,
                           samples=None, masks=None):
    """oracle.vanilla.render stage by stage with the oracle's own samplers, MLP and composite: at each level the rows of the
    samples that the fp32 BOX KEEP RULE skips are zero BEFORE the transmittance, level 1 - with `coarse` also level 0 - stops by the
    MODE-0 STOP RULE on those rows, and the rows behind the stop are zero before the composite.  samples = (t0, t1): the positions
    are GIVEN (oracle.vanilla.render's own `samples=`); masks = (m0, m1): the evaluated sets are GIVEN and no rule is applied.
    Returns ([(rgb, acc, depth)] * 2, [dict(t, w, keep, stop, T, T64, rows)] * 2)."""
    o, vd, rd = b["rays_o"], b["viewdirs"], b["rays_d"]
    n_coarse, n_fine = counts
    dir_enc = oracle.encoding.pos_enc(vd, 0, 4)
    out, extra = [], []
    t = w = None
    for level, prefix in enumerate(("coarse_mlp.", "fine_mlp.")):
        if samples is not None:
            t = samples[level]
            pts = oracle.sampling.points_on_rays(t, o, vd)
        elif level == 0:
            t, pts = oracle.sampling.vanilla_level0(o, vd, n_coarse, NEAR, FAR)
        else:
            mids = 0.5 * (t[..., 1:] + t[..., :-1])
            t, pts = oracle.sampling.vanilla_level1(mids, w[..., 1:-1], o, vd, t, n_fine)
        raw_rgb, raw_sigma = oracle.mlp.vanilla_mlp(params, prefix, oracle.encoding.pos_enc(pts, 0, 10), dir_enc)
        rows = torch.cat([oracle.mlp.colour_activation(raw_rgb), oracle.mlp.density_activation(raw_sigma)], dim=-1)
        N = t.shape[-1]
        if masks is not None:
            kept = masks[level]
            stop = torch.full((o.shape[0],), N, dtype=torch.long)
        else:
            kept = keep_rule_box(occ, box, o, vd, t, clip)
        rows = torch.where(kept[..., None], rows, torch.zeros_like(rows))
        T = transmittance0(rows[..., 3], t, rd)
        T64 = transmittance0(rows[..., 3], t, rd, torch.float64)
        if masks is None:
            if level == 1 or coarse:
                stop, _ = stops(T, eps, segment)
            else:
                stop = torch.full((o.shape[0],), N, dtype=torch.long)
            rows = zero_behind(rows, stop)
        comp, acc, w, depth = oracle.compositing.vanilla_composite(rows[..., :3], rows[..., 3:], t, rd, white_bkgd)
        out.append((comp, acc, depth))
        extra.append(dict(t=t, w=w, keep=kept, stop=stop, T=T, T64=T64, rows=rows))
    return out, extra


_FRAMES = {}


def oracle_frames(counts, n, eps=EPS, **kw):
    """(plain at eps = 0, marched at eps, extra of the marched frame) of the n strided rays on the oracle, cached."""
    key = (counts, n, eps, tuple(sorted(kw.items())))
    if key not in _FRAMES:
        b = rays(n)
        plain, _ = oracle_render_marching(state(counts), b, counts, 0.0, **kw)
        got, extra = oracle_render_marching(state(counts), b, counts, eps, **kw)
        _FRAMES[key] = (plain, got, extra)
    return _FRAMES[key]
