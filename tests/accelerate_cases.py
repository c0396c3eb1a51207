"""Shared inputs and restatements of the accelerated-frame tests (tests/test_accelerate_cpu.py, tests/test_gpu_accelerate.py):
occupancy skipping and early ray termination together (include/neo360_hip.h: ACCELERATED FRAME).

Scene, rays and sample counts are those of tests/terminate_cases.py (cases.small_scene() seen by cases.strided_rays(n), 64 + 70
samples = 65 and 135 per ray, segment 64); the grids are those of tests/occupancy_cases.py.  The two OPERATING POINTS are fixed
HERE, on the CPU oracle, on 96 rays - tests/test_accelerate_cpu.py asserts the mixes below, so that the GPU tests cannot pass
vacuously:

    A   oc.box_cells(32), density bias +6, eps 0.33   level-1 stops 64 (12 rays), 128 (54), 135 (30); 66 rays culled, 30 survive;
                                                      4,975 skipped samples in front of the stops; with coarse=True the level-0
                                                      stops are 64 (66 rays) and 65 (30)
    B   oc.mixed(32),     density bias +6, eps 1e-2   level-1 stops 128 (42), 135 (54); 54 rays culled; 3,064 skipped samples in
                                                      front of the stops

At both points no ray's fp64 boundary transmittance lies within tc.NEAR_TOL * eps of eps and no sample within oc.FACE_TOL of a
cell face.  Nothing here depends on the GPU.
"""
import torch

import occupancy_cases as oc
import oracle
import terminate_cases as tc

N_COARSE, N_FINE, SEGMENT = tc.N_COARSE, tc.N_FINE, tc.SEGMENT
BIAS = 6.0
POINTS = {
    "A": dict(grid=lambda: oc.box_cells(32), eps=0.33),
    "B": dict(grid=lambda: oc.mixed(32), eps=1e-2),
}


def state():
    return tc.state(BIAS)


def oracle_render_accelerated(params, rays, scene, occ, eps, segment=SEGMENT, coarse=False, n_coarse=N_COARSE, n_fine=N_FINE,
                              keep=False):
    """tc.oracle_render_terminating with the rows of the samples that the fp32 KEEP RULE (oc.keep_rule) skips set to zero BEFORE
    the transmittance and the composite, at both levels: the stops are the STOP RULE on the masked rows.  occ None: no grid.
    Returns the two level tuples; with keep also per level dict(fg_t, bg_s, fg_w, fg_keep, stop, T, T64, far, culled)."""
    o, d = rays["rays_o"], rays["rays_d"]
    near = torch.full_like(o[..., -1:], 1e-4)
    far, _ = oracle.rays.sphere_exit_depth(o, d)
    parts, extra = [], []
    fg_t = bg_s = fg_w = bg_w = None
    for level in range(2):
        if level == 0:
            fg_t, _ = oracle.sampling.neo_fg_level0(o, d, n_coarse, near, far)
            bg_s, _, _ = oracle.sampling.neo_bg_level0(o, d, n_coarse, far, 3.0)
            fg_name, bg_name = "fg_coarse_mlp.", "bg_coarse_mlp."
        else:
            fg_mid = 0.5 * (fg_t[..., 1:] + fg_t[..., :-1])
            bg_mid = 0.5 * (bg_s[..., 1:] + bg_s[..., :-1])
            fg_t, _ = oracle.sampling.neo_fg_level1(fg_mid, fg_w[..., 1:-1], o, d, fg_t, n_fine)
            bg_s, _, _ = oracle.sampling.neo_bg_level1(bg_mid, bg_w[..., 1:-1], o, d, bg_s, n_fine, far, 3.0)
            fg_name, bg_name = "fg_fine_mlp.", "bg_fine_mlp."
        fg_rgb, fg_sigma = oracle.neo360.region_eval(params, fg_name, rays, scene, fg_t, True)
        bg_rgb, bg_sigma = oracle.neo360.region_eval(params, bg_name, rays, scene, bg_s, False, far)
        N = fg_t.shape[-1]
        kept = oc.keep_rule(occ, o, d, fg_t)
        rows = torch.cat([fg_rgb, fg_sigma], dim=-1)
        rows = torch.where(kept[..., None], rows, torch.zeros_like(rows))
        T = tc.transmittance(rows[..., 3], fg_t, d, far)
        T64 = tc.transmittance(rows[..., 3], fg_t, d, far, torch.float64)
        if level == 1 or coarse:
            stop, _ = tc.stops(T, eps, segment)
        else:
            stop = torch.full((o.shape[0],), N, dtype=torch.long)
        rows = tc.zero_behind(rows, stop)
        fg_c, fg_acc, fg_w, lam, fg_depth = oracle.compositing.neo_composite(rows[..., :3], rows[..., 3:], fg_t, d, True, far, False)
        bg_c, _, bg_w, _, bg_depth = oracle.compositing.neo_composite(bg_rgb, bg_sigma, bg_s, d, False, None, False)
        parts.append((fg_c, fg_acc, lam, fg_depth, bg_c, bg_depth))
        extra.append(dict(fg_t=fg_t, bg_s=bg_s, fg_w=fg_w, fg_keep=kept, stop=stop, T=T, T64=T64, far=far))
    culled = (parts[0][2].squeeze(-1) < eps) & (parts[1][2].squeeze(-1) < eps)
    out = []
    for fg_c, fg_acc, lam, fg_depth, bg_c, bg_depth in parts:
        bg_c = torch.where(culled[:, None], torch.zeros_like(bg_c), bg_c)
        rgb = torch.where(culled[:, None], fg_c, fg_c + lam * bg_c)
        depth = torch.where(culled, fg_depth, fg_depth + lam.squeeze(-1) * bg_depth)
        out.append((rgb, fg_c, bg_c, fg_acc, lam, depth))
    for e in extra:
        e["culled"] = culled
    return (out, extra) if keep else out


def skipped_in_front(extra):
    """The level-1 samples that the grid skips in front of the ray's stop: work the grid saves that the stop would not."""
    e = extra[1]
    j = torch.arange(e["fg_keep"].shape[1])
    return int((~e["fg_keep"] & (j[None, :] < e["stop"][:, None])).sum())


def stop_counts(stop):
    """{stop value: rays} of a (R,) stop tensor."""
    values, counts = torch.unique(stop.cpu().long(), return_counts=True)
    return {int(v): int(c) for v, c in zip(values, counts)}


_FRAMES = {}


def oracle_frames(point, n=96, coarse=False):
    """The accelerated oracle frame of an operating point on the n strided rays, cached: (got, extra)."""
    key = (point, n, coarse)
    if key not in _FRAMES:
        p = POINTS[point]
        _FRAMES[key] = oracle_render_accelerated(state(), tc.rays(n), tc.scene(), p["grid"](), p["eps"], coarse=coarse, keep=True)
    return _FRAMES[key]
