"""Shared inputs and restatements of the PixelNeRF marching-frame tests (tests/test_pix_march_cpu.py, tests/test_gpu_pix_march.py;
include/neo360_hip.h: PIXELNERF MARCHING FRAME).  Nothing here depends on the GPU.

Inputs.  cases.small_scene(), synth.pixelnerf_state(0) with the density-layer bias of both MLPs raised by BIAS[counts], seen by
cases.neo_batch(cases.strided_rays(R)) between NEAR = 0.2 and FAR = 2.5.  BIAS is fixed HERE, by bisection on the CPU oracle at
eps = EPS (the synthetic MLP is close to a uniform fog, so one bias per count pair is needed): for every pair whose level 1 is
longer than one segment and every R >= 63 at least a quarter of the rays stop before N1 and at least a quarter never stop - on
the frame STOP_GRID names for the pair - which tests/test_pix_march_cpu.py asserts - so the GPU tests of the stop rule cannot pass vacuously.  The restated rules (the BOX KEEP
RULE, the MODE-0 STOP RULE, the boxes and grids) are those of tests/vanilla_march_cases.py, imported as they are; positions lie
along rays_d here.

    q1_index / q1_dirs       the direction a dense row is seen along: ray c0 + ((b - c0) N + j) mod bc of its reference chunk
    oracle_render_marching   oracle.pixelnerf.region_eval + oracle.compositing.vanilla_composite + oracle.sampling.vanilla_level0/1,
                             stage by stage, with the rows of the samples that are not evaluated zeroed before their composite
"""
import torch

import cases
import oracle
import vanilla_march_cases as vc
from neo360_amd import synth

keep_rule_box, transmittance0, stops, zero_behind, front = vc.keep_rule_box, vc.transmittance0, vc.stops, vc.zero_behind, vc.front
ball, n_level = vc.ball, vc.n_level
BOX, SMALL, FAR_AWAY = vc.BOX, vc.SMALL, vc.FAR_AWAY

# One bias per count pair, found by bisection on the CPU oracle.  3 + 4 has one segment: nothing can stop.
# 63 + 64 has NO robust bias on the unmasked frame: the 64th of the 128 merged samples is reached after about half of the fine
# samples, whatever the density, so only a fog that is opaque within the first coarse intervals stops there, and in a uniform fog
# all rays cross eps together (a bias of 51.79 stops 4 % of 257 rays, 51.88 stops 75 %).  For that pair the spread comes from the
# zero rows of a mixed grid instead (STOP_GRID): how far a ray's transmittance has fallen at the boundary then depends on how many
# of its samples the grid kept, and between a bias of 80 and 110 the stopped share moves only between 0.37 and 0.60.
BIAS = {(3, 4): 5.7, (7, 64): 5.7, (63, 64): 90.0, (64, 128): 1.95}
# The frame on which a pair's rays mix stopped and never-stopped ones: None - without a grid; (G, radius) - with the grid
# mixed(G, radius) over BOX and clip=True.
STOP_GRID = {(7, 64): None, (63, 64): (32, 0.45), (64, 128): None}
EPS = 1e-2
NEAR, FAR = 0.2, 2.5
SEGMENT = 64
COUNTS = ((3, 4), (7, 64), (63, 64), (64, 128))
RAYS = (1, 63, 64, 65, 257)
STOPPING = tuple(c for c in COUNTS if n_level(c)[1] > SEGMENT)
PER_RAY = ("rays_o", "rays_d", "viewdirs")

_SCENE = []


def mixed(G, radius=0.55):
    """vc.mixed with the ball's radius as a parameter (0.55: vc.mixed itself): a centred ball united with a 3-D checkerboard."""
    return ball(G, radius) | vc.oc.checkerboard(G)


def scene():
    if not _SCENE:
        _SCENE.append(cases.small_scene())
    return _SCENE[0]


def state(bias):
    """synth.pixelnerf_state(0) with both density-layer biases raised by `bias` (a number, or a count pair: its entry of BIAS)."""
    if isinstance(bias, tuple):
        bias = BIAS[bias]
    st = synth.pixelnerf_state(0)
    for k in ("coarse_mlp.density_layer.bias", "fine_mlp.density_layer.bias"):
        st[k] = st[k] + bias
    return st


def rays(n):
    return cases.neo_batch(cases.strided_rays(n))


def part(b, i, j):
    """Rays i .. j - 1 of a batch, the source cameras whole."""
    return {k: (v[i:j] if k in PER_RAY else v) for k, v in b.items()}


def q1_index(B, N, chunk=None):
    """(B,N) long: the ray whose direction sample j of ray b is seen along in a dense launch of B rays x N samples in reference
    chunks of `chunk` rays (None: one chunk) - c0 + ((b - c0) N + j) mod bc, [c0, c0 + bc) the chunk of b (the last may be short)."""
    chunk = B if chunk is None else chunk
    b = torch.arange(B)[:, None]
    j = torch.arange(N)[None, :]
    c0 = (b // chunk) * chunk
    bc = torch.clamp(B - c0, max=chunk)
    return c0 + ((b - c0) * N + j) % bc


def q1_dirs(viewdirs, N, chunk=None):
    """(B,N,3): viewdirs at q1_index."""
    return viewdirs[q1_index(viewdirs.shape[0], N, chunk).to(viewdirs.device)]


def oracle_rows(params, prefix, b, t):
    """(B,N,4) = (rgb, sigma) of oracle.pixelnerf.region_eval at the positions t: all rays of b as ONE reference chunk."""
    rgb, sigma = oracle.pixelnerf.region_eval(params, prefix, b, scene(), t)
    return torch.cat([rgb, sigma], dim=-1)


def oracle_render_marching(params, b, counts, eps, occ=None, box=None, clip=False, segment=SEGMENT, coarse=False, white_bkgd=False,
                           samples=None, masks=None):
    """oracle.pixelnerf.render stage by stage with the oracle's own samplers, evaluator and composite: at each level the rows of the
    samples that the fp32 BOX KEEP RULE (dirs = rays_d) skips are zero BEFORE the transmittance, level 1 - with `coarse` also level
    0 - stops by the MODE-0 STOP RULE on those rows, and the rows behind the stop are zero before the composite.  The rows are
    evaluated DENSE and then masked, so a masked frame's row is seen along the dense row's direction.  samples = (t0, t1): the
    positions are GIVEN; masks = (m0, m1): the evaluated sets are GIVEN and no rule is applied.
    Returns ([(rgb, acc, depth)] * 2, [dict(t, w, keep, stop, T, T64, rows)] * 2)."""
    o, rd = b["rays_o"], b["rays_d"]
    n_coarse, n_fine = counts
    out, extra = [], []
    t = w = None
    for level, prefix in enumerate(("coarse_mlp.", "fine_mlp.")):
        if samples is not None:
            t = samples[level]
        elif level == 0:
            t, _ = oracle.sampling.vanilla_level0(o, rd, n_coarse, NEAR, FAR)
        else:
            mids = 0.5 * (t[..., 1:] + t[..., :-1])
            t, _ = oracle.sampling.vanilla_level1(mids, w[..., 1:-1], o, rd, t, n_fine)
        rows = oracle_rows(params, prefix, b, t)
        N = t.shape[-1]
        if masks is not None:
            kept = masks[level]
            stop = torch.full((o.shape[0],), N, dtype=torch.long)
        else:
            kept = keep_rule_box(occ, box, o, rd, t, clip)
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


def oracle_frame(counts, n, eps=EPS, G=None, radius=0.55):
    """(outputs, extra) of the marched frame of the n strided rays on the oracle, cached.  G: with the grid mixed(G, radius) over BOX
    and clip=True; None: without a grid."""
    key = (counts, n, eps, G, radius)
    if key not in _FRAMES:
        kw = dict(occ=mixed(G, radius), box=BOX, clip=True) if G is not None else {}
        _FRAMES[key] = oracle_render_marching(state(counts), rays(n), counts, eps, **kw)
    return _FRAMES[key]
