"""Shared inputs of the instance-render tests (tests/test_instances_cpu.py, tests/test_gpu_instances.py).

Scene, state (density bias +6), BOX_A and BOX_B are those of tests/object_cases.py.  Three more boxes in the reference's `RTs`
format, and a seven-instance list with an empty instance and two exact duplicates:

    box F   R = rot_z(0.4) . rot_x(-0.3)   T = (0.29, 0.18, 0.18)   half-extents (0.06, 0.06, 0.02)
    box G   R = rot_z(0.8)                 T = (0.10, 0.02, 0.02)   half-extents (0.10, 0.16, 0.10)
    box D   R = identity                   T = (0, 0, 0.9)          0.03 cube          (no ray meets it)
    INSTANCES = [A, B, F, G, D, A, G]

Per-instance near / far come from the CPU oracle one box at a time (oracle.rays.sample_rays_in_bbox through object_cases.batch),
the per-instance renders from object_cases.oracle_render, so nothing here depends on the GPU.

`composite` is the torch fp32 restatement of the instance composite (include/neo360_hip.h, COMPOSITE RECURRENCE): eager torch
multiplies and adds separately, like the library built with -ffp-contract=off.
"""
import numpy as np
import torch

import object_cases as oc

BOX_A, BOX_B = oc.BOX_A, oc.BOX_B
BOX_F = dict(R=oc._rot_z(0.4) @ oc._rot_x(-0.3), T=np.array([0.29, 0.18, 0.18]), s=oc._bounds((0.06, 0.06, 0.02)))
BOX_G = dict(R=oc._rot_z(0.8), T=np.array([0.10, 0.02, 0.02]), s=oc._bounds((0.10, 0.16, 0.10)))
BOX_D = dict(R=np.eye(3), T=np.array([0.0, 0.0, 0.9]), s=oc._bounds(0.03))

DISTINCT = (BOX_A, BOX_B, BOX_F, BOX_G, BOX_D)
NAMES = "ABFGD"
INSTANCES = (BOX_A, BOX_B, BOX_F, BOX_G, BOX_D, BOX_A, BOX_G)
A, B, F, G, D = range(5)          # indices into DISTINCT, and of the first copy of each box in INSTANCES

N_COARSE, N_FINE = 16, 32


def index_of(box):
    return next(i for i, b in enumerate(DISTINCT) if b is box)


def rays(n):
    """The CPU batch of cases.strided_rays(n) without any interval keys."""
    b, _ = oc.batch(n, BOX_A)
    return {k: v for k, v in b.items() if k not in ("near_obj", "far_obj")}


def bounds(n, instances=INSTANCES):
    """near (K,n), far (K,n) float32 and hit (K,n) bool of CPU rays: the CPU oracle's single-box calls, stacked."""
    near, far, hit = [], [], []
    for box in instances:
        b, mask = oc.batch(n, box)
        near.append(b["near_obj"].reshape(-1))
        far.append(b["far_obj"].reshape(-1))
        hit.append(mask)
    if not near:
        return torch.zeros(0, n), torch.zeros(0, n), torch.zeros(0, n, dtype=torch.bool)
    return torch.stack(near), torch.stack(far), torch.stack(hit)


_ORACLE = {}


def oracle_instances(n, chunk=None):
    """The CPU oracle of the per-instance renders of the five distinct boxes at 16 + 32 samples, black background, cached:
    dict(near, far, hit (5,n), rgb0, acc0, depth0, rgb1, acc1, depth1 (5,n[,3])); rows without `hit` are zero."""
    key = (n, chunk)
    if key not in _ORACLE:
        near, far, hit = bounds(n, DISTINCT)
        b = rays(n)
        out = {k: [] for k in ("rgb0", "acc0", "depth0", "rgb1", "acc1", "depth1")}
        for i in range(len(DISTINCT)):
            if bool(hit[i].any()):
                o = oc.oracle_render(oc.state(), b, near[i], far[i], N_COARSE, N_FINE, white_bkgd=False, chunk=chunk)
            else:
                o = dict(rgb0=torch.zeros(n, 3), rgb1=torch.zeros(n, 3), acc0=torch.zeros(n), acc1=torch.zeros(n),
                         depth0=torch.zeros(n), depth1=torch.zeros(n))
            for k in out:
                m = hit[i].reshape((n,) + (1,) * (o[k].dim() - 1))
                out[k].append(torch.where(m, o[k].float(), torch.zeros_like(o[k].float())))
        _ORACLE[key] = dict(near=near, far=far, hit=hit, **{k: torch.stack(v) for k, v in out.items()})
    return _ORACLE[key]


def composite(near, far, p, a, d, white):
    """near, far, a, d (K,B), p (K,B,3) fp32 on any device -> rgb (B,3), acc (B,), depth (B,), id (B,) int32, and the per-ray
    order (K,B) with its validity, in plain fp32: hit instances in ascending lo (ties to the lower index), T = 1; v = T a;
    rgb += T p; depth += T d; acc += v; v > best -> best = v, id = i; T = T (1 - a); then rgb += 1 - acc when white."""
    K, Bn = near.shape
    dev = near.device
    lo, _, hit = oc.hit_rule(near.float(), far.float())
    key = torch.where(hit, lo, torch.full_like(lo, float("inf")))
    order = torch.sort(key, dim=0, stable=True).indices if K else torch.zeros(0, Bn, dtype=torch.long, device=dev)
    T = torch.ones(Bn, device=dev)
    rgb = torch.zeros(Bn, 3, device=dev)
    depth = torch.zeros(Bn, device=dev)
    acc = torch.zeros(Bn, device=dev)
    best = torch.zeros(Bn, device=dev)
    ids = torch.full((Bn,), -1, dtype=torch.int32, device=dev)
    cols = torch.arange(Bn, device=dev)
    valid = torch.zeros(K, Bn, dtype=torch.bool, device=dev)
    for s in range(K):
        i = order[s]
        ok = hit[i, cols]
        valid[s] = ok
        ai, di, pi = a[i, cols].float(), d[i, cols].float(), p[i, cols].float()
        v = T * ai
        rgb = torch.where(ok[:, None], rgb + T[:, None] * pi, rgb)
        depth = torch.where(ok, depth + T * di, depth)
        acc = torch.where(ok, acc + v, acc)
        win = ok & (v > best)
        best = torch.where(win, v, best)
        ids = torch.where(win, i.to(torch.int32), ids)
        T = torch.where(ok, T * (1.0 - ai), T)
    if white:
        rgb = rgb + (1.0 - acc)[:, None]
    return rgb, acc, depth, ids, order, valid
