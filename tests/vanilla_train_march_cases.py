"""Shared inputs and restatements of the tests of training through the vanilla occupancy grid
(tests/test_vanilla_train_march_cpu.py, tests/test_gpu_vanilla_train_march.py; include/neo360_hip.h: VANILLA MARCHING TRAINING).
Nothing here depends on the GPU.  The scene, rays, boxes and grids are those of tests/vanilla_march_cases.py, imported as they are.

    COUNTS / RAYS / GRIDS    the shapes of the issue: (3,4), (16,24), (7,64); 1, 63, 64, 65, 257 rays; G in {8, 32}
    state()                  synth.vanilla_state(0), as the training tests of the vanilla module use it (no density bias)
    level0()                 the deterministic level-0 positions of training.nerf_render_train
    counted_case()           rays and positions of which exactly `want` lie inside vc.SMALL (the exact kept counts of the row builder)
    probe_points()           the probe formula of neo_vanilla_grid_probes restated in torch, from given uniforms
    mse2()                   the reference's two-level MSE loss
"""
import torch

import vanilla_march_cases as vc
from neo360_amd import synth

COUNTS = ((3, 4), (16, 24), (7, 64))
RAYS = vc.RAYS
GRIDS = (8, 32)
EXACT = (0, 1, 63, 64, 65, 255, 256, 257, None)      # None: all
EXACT_SHAPE = (257, 8)                                  # the 250 of these rays that cross vc.SMALL x 8 = 2000 samples: two workgroups


def state():
    return synth.vanilla_state(0)


def level0(counts, n, near=vc.NEAR, far=vc.FAR):
    """(n, n_coarse + 1): helper.py:424-429 as training.nerf_render_train states it (randomized=False)."""
    lin = torch.linspace(0.0, 1.0, counts[0] + 1)
    edges = float(near) * (1.0 - lin) + float(far) * lin
    return edges[None, :].expand(n, counts[0] + 1).contiguous()


def counted_case(want, shape=EXACT_SHAPE, seed=3):
    """(rays, t (R',N), kept) of which exactly `kept` = want (None: all R' N) samples lie inside vc.SMALL: the rays of
    vc.rays(R) that cross vc.SMALL at all - at one of the positions of a scan of [NEAR, FAR] in steps of 0.01, by the fp32 rule -,
    `want` samples at flat positions drawn without replacement sitting at the middle one of their ray's inside positions, and
    every other sample at t = 50, far outside the box."""
    R, N = shape
    b = vc.rays(R)
    scan = torch.linspace(vc.NEAR, vc.FAR, 281)[None, :].expand(R, 281).contiguous()
    inside = vc.keep_rule_box(torch.ones(8, 8, 8, dtype=torch.bool), vc.SMALL, b["rays_o"], b["viewdirs"], scan, True)
    hit = inside.any(dim=1)
    b = {k: v[hit].contiguous() for k, v in b.items()}
    inside, scan = inside[hit], scan[hit]
    R = int(hit.sum())
    want = R * N if want is None else want
    assert R * N > 1024 and want <= R * N, "more than one workgroup of the compaction"
    first = inside.float().argmax(dim=1)
    mid = first + (inside.sum(dim=1) - 1) // 2      # the inside positions of a ray through a box are consecutive
    t_in = scan[torch.arange(R), mid]
    g = torch.Generator().manual_seed(seed)
    pick = torch.zeros(R * N, dtype=torch.bool)
    pick[torch.randperm(R * N, generator=g)[:want]] = True
    return b, torch.where(pick.reshape(R, N), t_in[:, None].expand(R, N), torch.full((R, N), 50.0)), want


def probe_points(box, G, u, dtype=torch.float64):
    """lo + (c + u) w per axis with w = (hi - lo) / G formed in fp32, evaluated in `dtype`; u (G^3, 3) in [0, 1).  Returns
    (pts (G^3, 3), cells (G^3, 3) as floats) in the grid's [ix][iy][iz] order."""
    lo = torch.tensor(box[0], dtype=torch.float32)
    hi = torch.tensor(box[1], dtype=torch.float32)
    w = (hi - lo) / torch.tensor(float(G), dtype=torch.float32)
    ax = torch.arange(G, dtype=dtype)
    cells = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3)
    return lo.to(dtype) + (cells + u.to(dtype)) * w.to(dtype), cells


def mse2(out, target):
    """vanilla_nerf/model.py:281-283: img2mse of the coarse and of the fine rgb."""
    return ((out[0][0] - target) ** 2).mean() + ((out[1][0] - target) ** 2).mean()


def grad_criterion(names, got, ref64, ref32):
    """The criterion of test_vanilla_training_step_gradients_vs_fp64_autograd: per tensor the library may miss fp64 by at most
    1.5 x what the fp32 oracle misses it by, + 2e-5, in max and in L2 (both relative to the fp64 gradient).  Returns the worst
    relative L2 error; raises AssertionError naming the tensor."""
    rel = lambda x, ref: (float(x.abs().max()) / (float(ref.abs().max()) + 1e-15), float(x.norm()) / (float(ref.norm()) + 1e-30))
    worst = 0.0
    for nm, a, b, r in zip(names, got, ref64, ref32):
        a = a.detach().cpu().double()
        lib, ref = rel(a - b, b), rel(r.double() - b, b)
        print("%-40s library max %.3e l2 %.3e | fp32 oracle max %.3e l2 %.3e" % (nm, lib[0], lib[1], ref[0], ref[1]))
        worst = max(worst, lib[1])
        assert lib[0] <= 1.5 * ref[0] + 2e-5 and lib[1] <= 1.5 * ref[1] + 2e-5, (nm, lib, ref)
    return worst
