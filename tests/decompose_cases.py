"""Shared restatements of the decomposed-render tests (tests/test_decompose_cpu.py, tests/test_gpu_decompose.py).

Scene, state (density bias +6), rays and the seven instances [A, B, F, G, D, A, G] are those of tests/instance_cases.py and
tests/edit_cases.py, at 16 + 32 samples.  Nothing here depends on the GPU.

    owners            the owner of every sample by the DECOMPOSITION RULE (include/neo360_hip.h): the smallest hit pair whose closed
                      interval holds it, else slot K;
    decompose_f64     the per-slot sums P_s, a_s, d_s in fp64 from fp32 inputs, and S_s = sum over the slot of w |x| for each of them
                      (the scale of the error bound);
    id_rule           the id map in fp32 from given fp32 masses - one fp32 add for rest_total, comparisons written so that a NaN
                      never wins.
"""
import torch

import edit_cases as ec
import instance_cases as ic

N_COARSE, N_FINE = ic.N_COARSE, ic.N_FINE
A, B, F, G, D = ic.A, ic.B, ic.F, ic.G, ic.D
K7 = len(ic.INSTANCES)


def owners(t, near, far):
    """t (R,N), near / far (K,R) on any device -> (R,N) int64: the smallest hit i with lo_i <= t_j <= hi_i, else K."""
    K = near.shape[0]
    inside = ec.inside_mask(t.float(), near, far)
    own = torch.full(t.shape, K, dtype=torch.long, device=t.device)
    for i in reversed(range(K)):
        own = torch.where(inside[i], torch.full_like(own, i), own)
    return own


def decompose_f64(rgbsigma, t, weights, near, far):
    """rgbsigma (R,N,4), t, weights (R,N), near / far (K,R), fp32 on any device (computed on the CPU in fp64).
    Returns dict(rgb (K+1,R,3), acc, depth (K+1,R)) and the same three keys with an `S_` prefix: sum over the slot of w |c|, w |1|
    and w |t| (|w| throughout), and own (R,N), count (K+1,R)."""
    rs, t, w = rgbsigma.detach().cpu().double(), t.detach().cpu().double(), weights.detach().cpu().double()
    near, far = near.detach().cpu(), far.detach().cpu()
    K = near.shape[0]
    own = owners(t.float(), near, far)
    out = {k: [] for k in ("rgb", "acc", "depth", "S_rgb", "S_acc", "S_depth", "count")}
    for s in range(K + 1):
        m = (own == s).double()
        ws = w * m
        out["rgb"].append((ws[..., None] * rs[..., :3]).sum(dim=1))
        out["acc"].append(ws.sum(dim=1))
        out["depth"].append((ws * t).sum(dim=1))
        out["S_rgb"].append((ws.abs()[..., None] * rs[..., :3].abs()).sum(dim=1))
        out["S_acc"].append(ws.abs().sum(dim=1))
        out["S_depth"].append((ws * t).abs().sum(dim=1))
        out["count"].append((own == s).sum(dim=1))
    res = {k: torch.stack(v) for k, v in out.items()}
    res["own"] = own
    return res


def id_rule(acc, bg_lambda=None):
    """acc (K+1,R) fp32 masses on any device, bg_lambda None, (R,) or (R,1) -> id (R,) int32 in fp32: rest_total = acc[K] + bg_lambda
    (one fp32 add), best = the largest acc[i], i < K, ties to the lower index, found as the kernel finds it (from best = 0, i
    ascending, `acc[i] > best`: a NaN never wins, and only a positive mass can); id = its index iff best > 0 and best >= rest_total."""
    acc = acc.float()
    K, R = acc.shape[0] - 1, acc.shape[1]
    rest = acc[K] if bg_lambda is None else acc[K] + bg_lambda.float().reshape(R)
    best = torch.zeros(R, device=acc.device)
    ids = torch.full((R,), -1, dtype=torch.int32, device=acc.device)
    for i in range(K):
        win = acc[i] > best
        best = torch.where(win, acc[i], best)
        ids = torch.where(win, torch.full_like(ids, i), ids)
    ok = (best > 0) & (best >= rest)
    return torch.where(ok, ids, torch.full_like(ids, -1))
