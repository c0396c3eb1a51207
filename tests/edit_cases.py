"""Shared inputs and restatements of the edited-render tests (tests/test_edit_cpu.py, tests/test_gpu_edit.py).

Scene, state (density bias +6), rays and the seven instances [A, B, F, G, D, A, G] are those of tests/instance_cases.py, at
16 + 32 samples.  Nothing here depends on the GPU.

    edit_rows               the torch fp32 restatement of the EDIT RULE (include/neo360_hip.h): eager torch multiplies one factor at
                            a time, like the kernel;
    composite_layers_f64    the fp64 restatement of the LAYER RECURRENCE from fp32 inputs;
    oracle_render_edited    the loop of oracle.neo360.render restated from region_eval, compositing.neo_composite and sampling.*,
                            with edit_rows before the foreground composite and optional given level-1 positions.
"""
import torch

import cases
import instance_cases as ic
import object_cases as oc
import oracle

N_COARSE, N_FINE = ic.N_COARSE, ic.N_FINE
A, B, F, G, D = ic.A, ic.B, ic.F, ic.G, ic.D
K7 = len(ic.INSTANCES)


def inside_mask(t, near, far):
    """t (R,N), near / far (K,R) -> (K,R,N) bool: sample j of a ray is inside pair i iff the pair is a hit and lo <= t_j <= hi."""
    lo, hi, hit = oc.hit_rule(near.float(), far.float())
    return hit[:, :, None] & (lo[:, :, None] <= t[None]) & (t[None] <= hi[:, :, None])


def edit_rows(rgbsigma, t, near, far, scale=None, tint=None):
    """rgbsigma (R,N,4), t (R,N), near / far (K,R) fp32 on any device; scale (K), tint (K,3) host sequences (None = ones).  For
    i = 0 .. K-1, samples inside pair i: sigma *= scale[i]; r *= tint[i][0]; g *= tint[i][1]; b *= tint[i][2], in fp32."""
    K = near.shape[0]
    out = rgbsigma.float().clone()
    inside = inside_mask(t.float(), near, far)
    for i in range(K):
        s = 1.0 if scale is None else float(scale[i])
        tr, tg, tb = (1.0, 1.0, 1.0) if tint is None else (float(x) for x in tint[i])
        fac = torch.tensor([tr, tg, tb, s], dtype=torch.float32, device=out.device)
        out = torch.where(inside[i][:, :, None], out * fac, out)
    return out


def composite_layers_f64(rgbsigma, t, rays_d, t_far, layers=None):
    """The LAYER RECURRENCE in fp64 from fp32 inputs (any device; computed on the CPU): rgbsigma (R,N,4), t (R,N), rays_d (R,3),
    t_far (R,) or (R,1); layers None or dict(key (L,R), rgb (L,R,3), acc (L,R), depth (L,R)).
    Returns dict(rgb (R,3), acc, depth (R,), weights (R,N) = the scene's own, bg_lambda (R,1), visibility (L,R)), float64."""
    rs, t, d = rgbsigma.detach().cpu().double(), t.detach().cpu().double(), rays_d.detach().cpu().double()
    far = t_far.detach().cpu().double().reshape(-1, 1)
    R, N = t.shape
    delta = torch.cat([t[:, 1:] - t[:, :-1], far - t[:, -1:]], dim=-1) * torch.norm(d, dim=-1, keepdim=True)
    alpha = 1.0 - torch.exp(-rs[..., 3] * delta)
    T = torch.cumprod(1.0 - alpha + 1e-10, dim=-1)
    S = torch.cat([torch.ones(R, 1, dtype=torch.float64), T[:, :-1]], dim=-1)        # exclusive
    S_end = T[:, -1]
    w_scene = alpha * S
    L = 0 if layers is None else layers["key"].shape[0]
    rgb = torch.zeros(R, 3, dtype=torch.float64)                  # the layers' share; the samples' is added below
    acc = torch.zeros(R, dtype=torch.float64)
    depth = torch.zeros(R, dtype=torch.float64)
    keeps = torch.ones(R, 1, dtype=torch.float64)
    front = torch.ones(R, N, dtype=torch.float64)                 # A(j)
    vis = torch.zeros(L, R, dtype=torch.float64)
    if L:
        key32, a32 = layers["key"].detach().cpu().float(), layers["acc"].detach().cpu().float()
        p, dl = layers["rgb"].detach().cpu().double(), layers["depth"].detach().cpu().double()
        keep32 = torch.clamp(1.0 - a32, min=0.0)                  # fp32, then widened
    for r in range(R):
        order = []
        if L:
            valid = torch.isfinite(key32[:, r]) & (a32[:, r] > 0)
            order = sorted((l for l in range(L) if bool(valid[l])), key=lambda l: (float(key32[l, r]), l))
        A = torch.ones(N, dtype=torch.float64)
        Bl = 1.0
        for l in order:
            k = float(key32[l, r])
            at = (t[r] >= k).nonzero().reshape(-1)
            s_here = float(S[r, at[0]]) if len(at) else float(S_end[r])
            v = s_here * Bl
            a = float(a32[l, r])
            rgb[r] += v * p[l, r]
            acc[r] += v * a
            depth[r] += v * float(dl[l, r])
            vis[l, r] = v * a
            keep = float(keep32[l, r])
            A = torch.where(t[r] >= k, A * keep, A)
            Bl = Bl * keep
        front[r] = A
        keeps[r, 0] = Bl
    # the samples' share in the form of oracle.compositing.neo_composite, so that L = 0 is exactly that function in fp64
    w = w_scene * front
    rgb = (w[..., None] * rs[..., :3]).sum(dim=-2) + rgb
    acc = w.sum(dim=-1) + acc
    depth = (w * t).sum(dim=-1) + depth
    return dict(rgb=rgb, acc=acc, depth=depth, weights=w_scene, bg_lambda=T[..., -1:] * keeps, visibility=vis)


def oracle_render_edited(params, rays, scene, near_inst, far_inst, scale=None, tint=None, n_coarse=N_COARSE, n_fine=N_FINE,
                         fine_samples=None, keep=False):
    """oracle.neo360.render(out_depth=True) restated stage by stage, with the fp32 edit on the foreground rows of each level before
    their composite.  rays: one reference chunk of CPU tensors.  fine_samples: None, or (fg_t, bg_s) level-1 rows to USE.
    Returns the two level tuples (rgb, fg_rgb, bg_rgb, fg_acc, bg_lambda, depth); with keep also per level dict(fg_t, bg_s, fg_w,
    fg_rows (the edited rows), fg_raw (before the edit))."""
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
        raw = torch.cat([fg_rgb, fg_sigma], dim=-1)
        rows = edit_rows(raw, fg_t, near_inst, far_inst, scale, tint).to(raw.dtype)
        fg_c, fg_acc, fg_w, lam, fg_depth = oracle.compositing.neo_composite(rows[..., :3], rows[..., 3:], fg_t, d, True, far, False)
        bg_c, _, bg_w, _, bg_depth = oracle.compositing.neo_composite(bg_rgb, bg_sigma, bg_s, d, False, None, False)
        out.append((fg_c + lam * bg_c, fg_c, bg_c, fg_acc, lam, fg_depth + lam.squeeze(-1) * bg_depth))
        extra.append(dict(fg_t=fg_t, bg_s=bg_s, fg_w=fg_w, fg_rows=rows, fg_raw=raw, far=far))
    return (out, extra) if keep else out


_LEVEL0 = {}


def oracle_level0(n):
    """The oracle's level-0 foreground sample rows (n, 17) of the n strided rays, cached: dict(fg_t, near, far, hit (7, n))."""
    if n not in _LEVEL0:
        b = ic.rays(n)
        o, d = b["rays_o"], b["rays_d"]
        far, _ = oracle.rays.sphere_exit_depth(o, d)
        fg_t, _ = oracle.sampling.neo_fg_level0(o, d, N_COARSE, torch.full_like(o[..., -1:], 1e-4), far)
        near7, far7, hit7 = ic.bounds(n)
        _LEVEL0[n] = dict(fg_t=fg_t, near=near7, far=far7, hit=hit7)
    return _LEVEL0[n]


def state():
    return oc.state()


def scene():
    return cases.small_scene()
