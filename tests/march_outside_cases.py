"""Shared inputs and restatements of the outside-sphere termination tests (tests/test_march_outside_cpu.py,
tests/test_gpu_march_outside.py).

Scene, rays, state, eps and sample counts are tests/terminate_cases.py's own, unchanged: cases.small_scene() seen by
cases.strided_rays(96), synth.nerf_tp_state(0) with both FOREGROUND density biases raised by 4 (the background is untouched),
EPS = 1e-2, 64 + 70 samples (65 and 135 per ray), segment 64.  On the CPU oracle 61 of the 96 rays are then culled and 35 survive,
and the survivors' level-1 outside stops are 64, 128 and N = 135 - asserted in tests/test_march_outside_cpu.py, so that the GPU
tests of the mixed frame cannot pass vacuously.  Nothing here depends on the GPU.

    transmittance_outside    the inclusive product T of the outside-sphere composite (oracle.compositing.neo_composite with
                             in_sphere=False: delta_i = s_i - s_{i+1}, the last one 1e10, no |d|), in the oracle's fp32 expressions or
                             restated in fp64 from the same fp32 rows; entry b - 1 is the transmittance in front of sample b;
    stops_outside            the OUTSIDE STOP RULE (include/neo360_hip.h) from such a T and the level's lambda: segment 0 always,
                             segment k >= 1 iff every earlier boundary b had !(lam * T[b - 1] < eps); returns stop and the value there;
    near_threshold_outside   the rays a fp32 and a fp64 statement of the rule may disagree on;
    oracle_render_marching   terminate_cases.oracle_render_terminating with the foreground of both levels first, the cull from its
                             lambdas, and the outside rows behind bg_stop zeroed before their composite.
"""
import torch

import oracle
import terminate_cases as tc

EPS = tc.EPS
SEGMENT = tc.SEGMENT
N_COARSE, N_FINE = tc.N_COARSE, tc.N_FINE
NEAR_TOL = tc.NEAR_TOL
BOUND = 1.003             # times eps: include/neo360_hip.h, MARCHING FRAME, BOUND


def transmittance_outside(sigma, s, dtype=torch.float32):
    """(R,N) inclusive product of 1 - alpha + 1e-10 of oracle.compositing.neo_composite(in_sphere=False), in `dtype` from the fp32
    inputs.  sigma (R,N), s (R,N) descending.  Entry b - 1 is the transmittance in front of sample b."""
    sigma, s = sigma.float().to(dtype), s.float().to(dtype)
    delta = torch.cat([s[..., :-1] - s[..., 1:], torch.full_like(s[..., :1], 1e10)], dim=-1)
    alpha = 1.0 - torch.exp(-sigma * delta)
    return torch.cumprod(1.0 - alpha + 1e-10, dim=-1)


def stops_outside(T, lam, eps, segment):
    """stop (R,) long and value (R,) = lam * T at the stop (lam * T[:, N - 1] where the march reaches N), in T's dtype: one
    multiply.  A NaN keeps marching."""
    R, N = T.shape
    lam = lam.reshape(R).to(T.dtype)
    stop = torch.full((R,), N, dtype=torch.long)
    value = lam * T[:, N - 1]
    alive = torch.ones(R, dtype=torch.bool)
    for b in tc.boundaries(N, segment):
        vb = lam * T[:, b - 1]
        halt = alive & (vb < eps)
        stop[halt] = b
        value[halt] = vb[halt]
        alive &= ~halt
    return stop, value


def near_threshold_outside(T64, lam, eps, segment):
    """(R,) bool: some boundary's fp64 running value lies within NEAR_TOL * eps of eps."""
    R, N = T64.shape
    lam = lam.reshape(R).double()
    out = torch.zeros(R, dtype=torch.bool)
    for b in tc.boundaries(N, segment):
        out |= (lam * T64[:, b - 1] - eps).abs() <= NEAR_TOL * eps
    return out


def threshold_distance(T64, lam, eps, segment):
    """(R,) the smallest |v_b - eps| / eps over the boundaries, in fp64 (inf without a boundary)."""
    R, N = T64.shape
    lam = lam.reshape(R).double()
    out = torch.full((R,), float("inf"), dtype=torch.float64)
    for b in tc.boundaries(N, segment):
        out = torch.minimum(out, (lam * T64[:, b - 1] - eps).abs() / eps)
    return out


def oracle_render_marching(params, rays, scene, eps, segment=SEGMENT, coarse=False, outside=True, n_coarse=N_COARSE, n_fine=N_FINE,
                           keep=False):
    """oracle.neo360.render(out_depth=True) restated stage by stage with the oracle's own composite, resampling and MLPs, in the
    launch order of the marching frame: the foreground of both levels (rows behind the inside stop zeroed, as
    terminate_cases.oracle_render_terminating), the cull from its two lambdas, then the background of both levels, in which - with
    `outside`, at level 1 and with `coarse` also at level 0 - the rows of a surviving ray behind bg_stop of the OUTSIDE STOP RULE (on
    the oracle's fp32 outside transmittance and the level's lambda, one fp32 multiply) are zero before their composite.  A culled ray
    has bg_stop = 0, bg_rgb = 0, rgb = fg_rgb, depth = fg_depth.  rays: one reference chunk of CPU tensors.  Returns the two level
    tuples; with keep also per level dict(fg_t, bg_s, fg_w, bg_w, stop, bg_stop, bg_value, T_bg, T64_bg, lam, far, culled)."""
    o, d = rays["rays_o"], rays["rays_d"]
    R = o.shape[0]
    near = torch.full_like(o[..., -1:], 1e-4)
    far, _ = oracle.rays.sphere_exit_depth(o, d)
    fg, extra = [], []
    fg_t = fg_w = None
    for level in range(2):
        if level == 0:
            fg_t, _ = oracle.sampling.neo_fg_level0(o, d, n_coarse, near, far)
        else:
            fg_mid = 0.5 * (fg_t[..., 1:] + fg_t[..., :-1])
            fg_t, _ = oracle.sampling.neo_fg_level1(fg_mid, fg_w[..., 1:-1], o, d, fg_t, n_fine)
        fg_rgb, fg_sigma = oracle.neo360.region_eval(params, "fg_coarse_mlp." if level == 0 else "fg_fine_mlp.", rays, scene, fg_t, True)
        N = fg_t.shape[-1]
        if level == 1 or coarse:
            stop, _ = tc.stops(tc.transmittance(fg_sigma[..., 0], fg_t, d, far), eps, segment)
        else:
            stop = torch.full((R,), N, dtype=torch.long)
        rows = tc.zero_behind(torch.cat([fg_rgb, fg_sigma], dim=-1), stop)
        fg_c, fg_acc, fg_w, lam, fg_depth = oracle.compositing.neo_composite(rows[..., :3], rows[..., 3:], fg_t, d, True, far, False)
        fg.append((fg_c, fg_acc, lam, fg_depth))
        extra.append(dict(fg_t=fg_t, fg_w=fg_w, stop=stop, far=far, lam=lam.squeeze(-1)))
    culled = (fg[0][2].squeeze(-1) < eps) & (fg[1][2].squeeze(-1) < eps)
    out = []
    bg_s = bg_w = None
    for level in range(2):
        if level == 0:
            bg_s, _, _ = oracle.sampling.neo_bg_level0(o, d, n_coarse, far, 3.0)
        else:
            bg_mid = 0.5 * (bg_s[..., 1:] + bg_s[..., :-1])
            bg_s, _, _ = oracle.sampling.neo_bg_level1(bg_mid, bg_w[..., 1:-1], o, d, bg_s, n_fine, far, 3.0)
        bg_rgb, bg_sigma = oracle.neo360.region_eval(params, "bg_coarse_mlp." if level == 0 else "bg_fine_mlp.", rays, scene, bg_s, False, far)
        N = bg_s.shape[-1]
        lam = extra[level]["lam"]
        T = transmittance_outside(bg_sigma[..., 0], bg_s)
        T64 = transmittance_outside(bg_sigma[..., 0], bg_s, torch.float64)
        if outside and (level == 1 or coarse):
            bg_stop, bg_value = stops_outside(T, lam, eps, segment)
        else:
            bg_stop, bg_value = torch.full((R,), N, dtype=torch.long), lam * T[:, N - 1]
        bg_stop = torch.where(culled, torch.zeros_like(bg_stop), bg_stop)
        bg_value = torch.where(culled, torch.zeros_like(bg_value), bg_value)
        rows = tc.zero_behind(torch.cat([bg_rgb, bg_sigma], dim=-1), torch.where(culled, torch.full_like(bg_stop, N), bg_stop))
        bg_c, _, bg_w, _, bg_depth = oracle.compositing.neo_composite(rows[..., :3], rows[..., 3:], bg_s, d, False, None, False)
        fg_c, fg_acc, lam2, fg_depth = fg[level]
        bg_c = torch.where(culled[:, None], torch.zeros_like(bg_c), bg_c)
        rgb = torch.where(culled[:, None], fg_c, fg_c + lam2 * bg_c)
        depth = torch.where(culled, fg_depth, fg_depth + lam2.squeeze(-1) * bg_depth)
        out.append((rgb, fg_c, bg_c, fg_acc, lam2, depth))
        extra[level].update(bg_s=bg_s, bg_w=bg_w, bg_stop=bg_stop, bg_value=bg_value, T_bg=T, T64_bg=T64, culled=culled)
    return (out, extra) if keep else out


_FRAMES = {}


def oracle_frames(n=96, eps=EPS, coarse=False):
    """The marching oracle frame of the n strided rays at N_COARSE + N_FINE without and with the outside rule, cached:
    (inside_only, got, extra) - inside_only is the same call with outside=False."""
    key = (n, eps, coarse)
    if key not in _FRAMES:
        b = tc.rays(n)
        inside_only = oracle_render_marching(tc.state(), b, tc.scene(), eps, coarse=coarse, outside=False)
        got, extra = oracle_render_marching(tc.state(), b, tc.scene(), eps, coarse=coarse, outside=True, keep=True)
        _FRAMES[key] = (inside_only, got, extra)
    return _FRAMES[key]
