"""Shared inputs and restatements of the empty-space-skipping tests (tests/test_occupancy_cpu.py, tests/test_gpu_occupancy.py).

Scene, state (density bias +6), rays and boxes are those of tests/instance_cases.py / tests/edit_cases.py, at 16 + 32 samples.
Nothing here depends on the GPU.

    positions / cell / keep_rule   the KEEP RULE (include/neo360_hip.h) in fp32 - eager torch adds and multiplies separately, like
                                   the library built with -ffp-contract=off - and in fp64 from the same fp32 inputs;
    near_face                      the samples the two may disagree on: within 2^-20 * 2 / G of a cell face on some axis;
    dilate / from_sigma            the grid construction: any probe not <= threshold, a (2 d + 1)^3 box maximum written as shifted
                                   ORs, the unit-sphere clip in integers;
    oracle_render_skipping         edit_cases.oracle_render_edited's restatement of oracle.neo360.render with the skipped rows zeroed
                                   before the foreground composite.
"""
import numpy as np
import torch

import edit_cases as ec
import instance_cases as ic
import oracle

N_COARSE, N_FINE = ec.N_COARSE, ec.N_FINE
FACE_TOL = 2.0 ** -20           # times the cell size 2 / G


def positions(rays_o, rays_d, t, dtype=torch.float32):
    """x = o + t d per sample, (B,N,3): one multiply and one add per coordinate in `dtype`, from the fp32 inputs."""
    o, d, t = (v.float().to(dtype) for v in (rays_o, rays_d, t))
    return o[:, None, :] + t[:, :, None] * d[:, None, :]


def cell(x, G):
    """min(max(floor((x + 1) * (G / 2)), 0), G - 1) per coordinate in x's own dtype; long.  Non-finite coordinates give cell 0."""
    half = torch.tensor(0.5 * G, dtype=x.dtype, device=x.device)
    c = torch.floor((x + 1.0) * half)
    c = torch.where(torch.isfinite(c), c, torch.zeros_like(c))
    return c.clamp(0, G - 1).long()


def keep_rule(occ, rays_o, rays_d, t, dtype=torch.float32):
    """(B,N) bool: the cell of x is set, or a coordinate of x is not finite, or occ is None."""
    x = positions(rays_o, rays_d, t, dtype)
    wild = ~torch.isfinite(x).all(dim=-1)
    if occ is None:
        return torch.ones_like(wild)
    c = cell(x, occ.shape[0])
    return occ.to(x.device)[c[..., 0], c[..., 1], c[..., 2]] | wild


def near_face(rays_o, rays_d, t, G):
    """(B,N) bool: a coordinate of the fp64 position lies within FACE_TOL * 2 / G of a cell face (FACE_TOL cells).  These samples
    are left out of every comparison of a keep mask with a restatement."""
    x = positions(rays_o, rays_d, t, torch.float64)
    u = (x + 1.0) * (0.5 * G)
    return ((u - torch.round(u)).abs() <= FACE_TOL).any(dim=-1) & torch.isfinite(x).all(dim=-1)


def dilate(occ, d):
    """bool (G,G,G): a cell is set iff a cell at most d away in every axis is set - d rounds of the 26-neighbourhood."""
    out = occ.clone()
    for _ in range(d):
        src = out.clone()
        G = src.shape[0]
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    xs, xd = (slice(max(dx, 0), G + min(dx, 0)), slice(max(-dx, 0), G + min(-dx, 0)))
                    ys, yd = (slice(max(dy, 0), G + min(dy, 0)), slice(max(-dy, 0), G + min(-dy, 0)))
                    zs, zd = (slice(max(dz, 0), G + min(dz, 0)), slice(max(-dz, 0), G + min(-dz, 0)))
                    out[xd, yd, zd] |= src[xs, ys, zs]
    return out


def sphere_cells(G):
    """bool (G,G,G): the cell has a point inside the closed unit sphere - n_x^2 + n_y^2 + n_z^2 <= h^2 with h = G / 2 and n = i - h
    for i >= h, h - 1 - i below."""
    h = G // 2
    i = torch.arange(G)
    n = torch.where(i >= h, i - h, h - 1 - i)
    return (n[:, None, None] ** 2 + n[None, :, None] ** 2 + n[None, None, :] ** 2) <= h * h


def from_sigma(sigma, G, probes, threshold, d):
    """The grid construction from an (M,M,M) lattice of densities, M = G * probes, on the CPU."""
    s = sigma.detach().cpu().float().reshape(G, probes, G, probes, G, probes)
    raw = (~(s <= threshold)).any(dim=5).any(dim=3).any(dim=1)
    return dilate(raw, d) & sphere_cells(G)


def ones(G):
    return torch.ones(G, G, G, dtype=torch.bool)


def zeros(G):
    return torch.zeros(G, G, G, dtype=torch.bool)


def checkerboard(G):
    i = torch.arange(G)
    return ((i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2) == 0


def box_cells(G, boxes=ic.DISTINCT):
    """bool (G,G,G): cells whose centre, in a box's frame, lies within the box grown by one cell - a superset of the cells the
    boxes meet."""
    c = (-1.0 + (torch.arange(G, dtype=torch.float64) + 0.5) * (2.0 / G))
    p = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), dim=-1).reshape(-1, 3)
    out = torch.zeros(G ** 3, dtype=torch.bool)
    for box in boxes:
        rot = torch.tensor(np.reshape(np.array(box["R"], dtype=np.float64), (3, 3)))
        tran = torch.tensor(np.array(box["T"], dtype=np.float64))
        b = torch.tensor(np.asarray(box["s"], dtype=np.float64).reshape(2, 3))
        q = (p - tran) @ rot                      # rows: R^T (p - T)
        out |= ((q >= b[0] - 2.0 / G) & (q <= b[1] + 2.0 / G)).all(dim=-1)
    return out.reshape(G, G, G)


def mixed(G=32):
    """The mixed grid of the tests: the cells around the five boxes, united with a 3-D checkerboard so that kept and skipped
    samples alternate along every ray and the compact tiles are ragged."""
    return box_cells(G) | checkerboard(G)


def oracle_render_skipping(params, rays, scene, occ, n_coarse=N_COARSE, n_fine=N_FINE, fine_samples=None, keep=False):
    """oracle.neo360.render(out_depth=True) restated stage by stage (edit_cases.oracle_render_edited, no edit), with the
    inside-sphere rows of the samples the fp32 KEEP RULE skips set to zero before their composite.  rays: one reference chunk of
    CPU tensors.  Returns the two level tuples; with keep also per level dict(fg_t, bg_s, fg_w, fg_keep)."""
    o, d = rays["rays_o"], rays["rays_d"]
    near = torch.full_like(o[..., -1:], 1e-4)
    far, _ = oracle.rays.sphere_exit_depth(o, d)
    out, extra = [], []
    fg_t = bg_s = fg_w = bg_w = None
    for level in range(2):
        if level == 0:
            fg_t, _ = oracle.sampling.neo_fg_level0(o, d, n_coarse, near, far)
            bg_s, _, _ = oracle.sampling.neo_bg_level0(o, d, n_coarse, far, 3.0)
            fg_name, bg_name = "fg_coarse_mlp.", "bg_coarse_mlp."
        else:
            if fine_samples is not None:
                fg_t, bg_s = fine_samples
            else:
                fg_mid = 0.5 * (fg_t[..., 1:] + fg_t[..., :-1])
                bg_mid = 0.5 * (bg_s[..., 1:] + bg_s[..., :-1])
                fg_t, _ = oracle.sampling.neo_fg_level1(fg_mid, fg_w[..., 1:-1], o, d, fg_t, n_fine)
                bg_s, _, _ = oracle.sampling.neo_bg_level1(bg_mid, bg_w[..., 1:-1], o, d, bg_s, n_fine, far, 3.0)
            fg_name, bg_name = "fg_fine_mlp.", "bg_fine_mlp."
        fg_rgb, fg_sigma = oracle.neo360.region_eval(params, fg_name, rays, scene, fg_t, True)
        bg_rgb, bg_sigma = oracle.neo360.region_eval(params, bg_name, rays, scene, bg_s, False, far)
        kept = keep_rule(occ, o, d, fg_t)
        rows = torch.cat([fg_rgb, fg_sigma], dim=-1)
        rows = torch.where(kept[..., None], rows, torch.zeros_like(rows))
        fg_c, fg_acc, fg_w, lam, fg_depth = oracle.compositing.neo_composite(rows[..., :3], rows[..., 3:], fg_t, d, True, far, False)
        bg_c, _, bg_w, _, bg_depth = oracle.compositing.neo_composite(bg_rgb, bg_sigma, bg_s, d, False, None, False)
        out.append((fg_c + lam * bg_c, fg_c, bg_c, fg_acc, lam, fg_depth + lam.squeeze(-1) * bg_depth))
        extra.append(dict(fg_t=fg_t, bg_s=bg_s, fg_w=fg_w, fg_keep=kept))
    return (out, extra) if keep else out


def classifier_case(R, N, G, seed, dyadic=True):
    """rays and sample rows of the classifier test: origins inside the sphere, directions of any length, t ascending in [0, 2.2] -
    so positions leave the cube on some rays (the clamp) - plus non-finite t and origins when there is room.
    dyadic: origins are multiples of 2^-12, directions and t of 2^-10, so every product and sum of the rule is EXACT in fp32 (x is a
    multiple of 2^-20 below 8: 23 bits) and the fp32 and fp64 restatements must agree on every sample, faces included; a sample
    then sits on a face of the finest grid (multiples of 2^-7) with probability 2^-13 per axis, far under the 1 % cap."""
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(R, 3, generator=g) - 0.5) * 1.2
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True) * (0.5 + torch.rand(R, 1, generator=g))
    t = torch.sort(torch.rand(R, N, generator=g) * 2.2, dim=-1).values
    if R >= 7:
        t[3, N // 2] = float("nan")
        t[4, 0] = float("inf")
        o[5, 1] = float("nan")
        o[6] = torch.tensor([-1.26, 1.51, 0.03])         # outside the cube on two axes: the clamp
        d[6] = torch.tensor([0.0, 0.0, 0.25])
    if dyadic:
        o, d, t = torch.round(o * 4096.0) / 4096.0, torch.round(d * 1024.0) / 1024.0, torch.round(t * 1024.0) / 1024.0
    occ = torch.rand(G, G, G, generator=g) < 0.4
    return occ, o, d, t
