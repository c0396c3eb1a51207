"""Shared inputs and restatements of the early-ray-termination tests (tests/test_terminate_cpu.py, tests/test_gpu_terminate.py).

Scene and rays are those of tests/edit_cases.py / tests/instance_cases.py (cases.small_scene() seen by cases.strided_rays(n)); the
state is synth.nerf_tp_state(0) with both foreground density biases raised by BIAS, as tests/test_gpu_cull_background._net does.
BIAS and EPS are fixed HERE, on the CPU oracle, at N_COARSE = 64 and N_FINE = 70 (65 and 135 samples, segment 64): the 96 rays
then show three different level-1 stops (64, 128 and N = 135) and both culled and surviving rays, which
tests/test_terminate_cpu.py asserts - so the GPU tests of the mixed frame cannot pass vacuously.  Nothing here depends on the GPU.

    transmittance            the inclusive product T of the inside-sphere composite, (1 - alpha + 1e-10) cumulated along the ray, in
                             the oracle's fp32 expressions or restated in fp64 from the same fp32 rows;
    stops                    the STOP RULE (include/neo360_hip.h) from such a T: segment 0 always, segment k >= 1 iff every earlier
                             boundary b had !(T[b - 1] < eps); returns stop (R,) and the transmittance at the stop;
    near_threshold           the rays a fp32 and a fp64 statement of the rule may disagree on: a boundary with |T - eps| <= 1e-5 eps;
    oracle_render_terminating  occupancy_cases.oracle_render_skipping's restatement of oracle.neo360.render with the rows behind
                             the stop zeroed before the foreground composite and the background of opaque rays dropped.
"""
import torch

import cases
import oracle
from neo360_amd import synth

BIAS = 4.0
EPS = 1e-2
N_COARSE, N_FINE = 64, 70
SEGMENT = 64
NEAR_TOL = 1e-5           # times eps


def state(bias=BIAS):
    st = synth.nerf_tp_state(0)
    for k in ("fg_coarse_mlp.density_layer.bias", "fg_fine_mlp.density_layer.bias"):
        st[k] = st[k] + bias
    return st


def scene():
    return cases.small_scene()


def rays(n):
    return cases.neo_batch(cases.strided_rays(n))


def transmittance(sigma, t, d, far, dtype=torch.float32):
    """(R,N) inclusive product of 1 - alpha + 1e-10 of oracle.compositing.neo_composite(in_sphere=True), in `dtype` from the fp32
    inputs.  sigma (R,N), t (R,N), d (R,3), far (R,1).  Entry b - 1 is the transmittance in front of sample b."""
    sigma, t, d, far = (v.float().to(dtype) for v in (sigma, t, d, far))
    delta = torch.cat([t[..., 1:] - t[..., :-1], far - t[..., -1:]], dim=-1)
    delta = delta * torch.norm(d[..., None, :], dim=-1)
    alpha = 1.0 - torch.exp(-sigma * delta)
    return torch.cumprod(1.0 - alpha + 1e-10, dim=-1)


def boundaries(N, segment):
    return list(range(segment, N, segment))


def stops(T, eps, segment):
    """stop (R,) long and trans (R,) = T at the stop (T[:, N - 1] where the march reaches N).  A NaN keeps marching."""
    R, N = T.shape
    stop = torch.full((R,), N, dtype=torch.long)
    trans = T[:, N - 1].clone()
    alive = torch.ones(R, dtype=torch.bool)
    for b in boundaries(N, segment):
        tb = T[:, b - 1]
        halt = alive & (tb < eps)
        stop[halt] = b
        trans[halt] = tb[halt]
        alive &= ~halt
    return stop, trans


def near_threshold(T64, eps, segment):
    """(R,) bool: some boundary's fp64 transmittance lies within NEAR_TOL * eps of eps."""
    R, N = T64.shape
    out = torch.zeros(R, dtype=torch.bool)
    for b in boundaries(N, segment):
        out |= (T64[:, b - 1] - eps).abs() <= NEAR_TOL * eps
    return out


def zero_behind(rows, stop):
    """rows (R,N,C) with the samples j >= stop[r] set to zero."""
    j = torch.arange(rows.shape[1], device=rows.device)
    return torch.where((j[None, :] < stop.to(rows.device)[:, None])[..., None], rows, torch.zeros_like(rows))


def oracle_render_terminating(params, rays, scene, eps, segment=SEGMENT, coarse=False, n_coarse=N_COARSE, n_fine=N_FINE, keep=False):
    """oracle.neo360.render(out_depth=True) restated stage by stage (occupancy_cases.oracle_render_skipping) with the oracle's own
    composite, resampling and MLPs: at level 1 - with `coarse` also at level 0 - the inside-sphere rows behind the stop of the
    STOP RULE (on the oracle's fp32 transmittance) are zero before their composite; a ray whose two bg_lambda are both below eps
    gets bg_rgb = 0, rgb = fg_rgb, depth = fg_depth.  rays: one reference chunk of CPU tensors.  Returns the two level tuples;
    with keep also per level dict(fg_t, bg_s, fg_w, stop, T (the fp32 transmittance of the full rows), T64, far) and `culled`."""
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
        T = transmittance(fg_sigma[..., 0], fg_t, d, far)
        T64 = transmittance(fg_sigma[..., 0], fg_t, d, far, torch.float64)
        if level == 1 or coarse:
            stop, _ = stops(T, eps, segment)
        else:
            stop = torch.full((o.shape[0],), N, dtype=torch.long)
        rows = zero_behind(torch.cat([fg_rgb, fg_sigma], dim=-1), stop)
        fg_c, fg_acc, fg_w, lam, fg_depth = oracle.compositing.neo_composite(rows[..., :3], rows[..., 3:], fg_t, d, True, far, False)
        bg_c, _, bg_w, _, bg_depth = oracle.compositing.neo_composite(bg_rgb, bg_sigma, bg_s, d, False, None, False)
        parts.append((fg_c, fg_acc, lam, fg_depth, bg_c, bg_depth))
        extra.append(dict(fg_t=fg_t, bg_s=bg_s, fg_w=fg_w, stop=stop, T=T, T64=T64, far=far))
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


_PLAIN = {}


def oracle_frames(n=96, eps=EPS, coarse=False):
    """The plain oracle frame and the terminating one of the n strided rays at N_COARSE + N_FINE, cached: (plain, got, extra)."""
    key = (n, eps, coarse)
    if key not in _PLAIN:
        b = rays(n)
        plain = oracle.neo360.render(state(), b, scene(), N_COARSE, N_FINE, out_depth=True)
        got, extra = oracle_render_terminating(state(), b, scene(), eps, coarse=coarse, keep=True)
        _PLAIN[key] = (plain, got, extra)
    return _PLAIN[key]
