"""Case table, CPU restatement and per-entry bounds for Mip-NeRF 360's two regularisers (training.lossfun_outer /
lossfun_distortion over neo_mip_lossfun_outer[_backward] / neo_mip_lossfun_distortion).  Plain CPU torch, in the style of
tests/alongray_cases.py: tests/test_mip_losses_cpu.py checks the restatement against the reference's own results
(tests/golden/g12_mip_losses.npz) and the conditions of every case; tests/test_gpu_mip_losses.py hands the same inputs to the kernels.

The restatement (mipnerf360/helper.py:108-148) is written for reading, not speed: the quadratic forms, any dtype, differentiable.

Shapes (N, Ne) sit on the edges of a 64-lane round and of the entry points' limits, R = 9 rays each, and the mid shape (128, 64) is
repeated at the ray counts of alongray_cases.RAY_COUNTS.  Two input families per shape:
  grid     edges = sorted integers out of 0 .. 4096 over 4096 with the ends forced to 0 and 1 (many ties and zero-width intervals),
           weights = integers 0 .. 64 over 4096 (zeros included), upstream gradient in eighths: every fp32 prefix sum is exact;
  random   sorted uniform edges, rand^3 weights normalised per row, and the degenerate rows 0 fine edges equal to envelope edges,
           1 a zero-width fine interval, 2 an envelope that dominates everywhere (loss and gradients exactly 0), 3 all-zero w,
           4 one spike among weights of 1e-9.

Bounds.  Every entry of every output is within DISTLOSS x max(1, largest |fp64 value| of that tensor in the case) of the fp64
restatement; DISTLOSS = 1e-6 is the constant the sibling kernel k_distloss is held to.  No entry is exempted and no noise term is
added: with fp64 between the fp32 inputs and outputs a result differs from the fp64 value by its final rounding (6e-8 relative).
The reference's own fp32 arithmetic meets the bound on the grid family (all five outputs) and, on the random family, for the loss
values, the distortion loss and its gradient; its fp32 lossfun_outer GRADIENTS do not (a difference of two fp32 cumulative sums
divided by w + eps: up to 0.27 absolute on g_w_env at scale 6.9), which is why FP32_INSIDE leaves them out for that family.
"""
import functools

import torch

from alongray_cases import DISTLOSS, RAY_COUNTS, assert_inside, scale_of, summarize, worst_entry  # noqa: F401

EPS = 1.1920929e-07             # helper.py:18
R_CASE = 9
SHAPES = ((1, 1), (2, 3), (3, 2), (32, 64), (63, 64), (64, 64), (65, 63), (128, 64), (129, 257), (385, 64), (64, 385), (1024, 1024))
FIXTURE_SHAPES = tuple(s for s in SHAPES if max(s) <= 385)
MID_SHAPE = (128, 64)
FAMILIES = ("grid", "random")
INPUTS = ("t", "w", "t_env", "w_env", "up", "up_dist")
OUTPUTS = ("loss", "g_w", "g_w_env", "dist", "g_dist")
# outputs on which the reference's fp32 arithmetic itself stays inside the bounds (module docstring)
FP32_INSIDE = {"grid": OUTPUTS, "random": ("loss", "dist", "g_dist")}


# ---- the two helpers, restated ---------------------------------------------------------------------------------------------------
def bracket(t, t_env):
    """searchsorted(t_env, t) of helper.py:108-113 for every fine edge: lo = the last envelope edge <= v (0 when there is none),
    hi = the first envelope edge > v (the last index when there is none).  With ub = #{envelope edges <= v} on sorted rows these
    are max(ub - 1, 0) and min(ub, Ne)."""
    ub = (t_env[..., None, :] <= t[..., :, None]).sum(-1)
    return torch.clamp(ub - 1, min=0), torch.clamp(ub, max=t_env.shape[-1] - 1)


def outer_weight(lo, hi, w_env):
    """y0_outer of inner_outer (helper.py:116-131): the envelope's weight from the bin holding a fine interval's left edge up to and
    including the bin holding its right edge, as a difference of the exclusive cumulative sum."""
    cy = torch.cat([torch.zeros_like(w_env[..., :1]), torch.cumsum(w_env, dim=-1)], dim=-1)
    return torch.gather(cy, -1, hi[..., 1:]) - torch.gather(cy, -1, lo[..., :-1])


def lossfun_outer(t, w, t_env, w_env, lo_hi=None):
    """helper.py:135-137.  lo_hi: a (lo, hi) pair in place of bracket(t, t_env) (the planted-error test)."""
    lo, hi = lo_hi if lo_hi is not None else bracket(t, t_env)
    return torch.clip(w - outer_weight(lo, hi, w_env), min=0) ** 2 / (w + EPS)


def lossfun_distortion(t, w):
    """helper.py:141-148: every pair of intervals at the distance of their midpoints, plus each interval against itself."""
    u = (t[..., 1:] + t[..., :-1]) / 2
    between = (w[..., :, None] * w[..., None, :] * (u[..., :, None] - u[..., None, :]).abs()).sum((-1, -2))
    within = (w ** 2 * (t[..., 1:] - t[..., :-1])).sum(-1) / 3
    return between + within


def interlevel_loss(history):
    """model.py:725-734 on a list of dict(sdist, weights)."""
    c, w = history[-1]["sdist"].detach(), history[-1]["weights"].detach()
    return sum(torch.mean(lossfun_outer(c, w, h["sdist"], h["weights"])) for h in history[:-1])


def distortion_loss(history):
    """model.py:736-741."""
    return torch.mean(lossfun_distortion(history[-1]["sdist"], history[-1]["weights"]))


def training_loss(rgb, history, target, data_loss_mult=1.0, interlevel_loss_mult=1.0, distortion_loss_mult=0.01, charb_padding=0.001):
    """model.py:439-449."""
    mse = torch.mean((rgb - target) ** 2)
    return (torch.sqrt(mse + charb_padding ** 2) * data_loss_mult + interlevel_loss(history) * interlevel_loss_mult
            + distortion_loss(history) * distortion_loss_mult)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _seed(N, Ne, R):
    return N * 1000 + Ne + (0 if R == R_CASE else 7919 * R)


def random_inputs(N, Ne, R=R_CASE):
    g = torch.Generator().manual_seed(_seed(N, Ne, R))
    te = torch.sort(torch.rand(R, Ne + 1, generator=g), -1).values
    te[:, 0], te[:, -1] = 0, 1
    t = torch.sort(torch.rand(R, N + 1, generator=g), -1).values
    t[:, 0], t[:, -1] = 0, 1
    k = min(N + 1, Ne + 1)
    if R > 0:
        t[0, :k] = te[0, :k]
        t[0] = torch.sort(t[0]).values
    if R > 1 and N >= 3:
        t[1, 1:3] = t[1, 1]
    w = torch.rand(R, N, generator=g) ** 3
    w = w / w.sum(-1, keepdim=True)
    we = torch.rand(R, Ne, generator=g) ** 3
    we = we / we.sum(-1, keepdim=True)
    if R > 2:
        we[2] = 1.0
    if R > 3:
        w[3] = 0.0
    if R > 4:
        w[4] = 1e-9
        w[4, N // 2] = 1.0
    return dict(t=t, w=w, t_env=te, w_env=we)


def grid_inputs(N, Ne, R=R_CASE):
    g = torch.Generator().manual_seed(_seed(N, Ne, R))

    def edges(n):
        e = torch.sort(torch.randint(0, 4097, (R, n + 1), generator=g), -1).values.float() / 4096
        e[:, 0], e[:, -1] = 0, 1
        return e

    t, te = edges(N), edges(Ne)
    w = torch.randint(0, 65, (R, N), generator=g).float() / 4096
    we = torch.randint(0, 65, (R, Ne), generator=g).float() / 4096
    return dict(t=t, w=w, t_env=te, w_env=we)


def upstream(R, N):
    """Upstream gradients of lossfun_outer (R, N), in eighths, and of lossfun_distortion (R,)."""
    g = torch.Generator().manual_seed(6)
    return dict(up=(torch.randint(1, 9, (R, N), generator=g) / 8).float(), up_dist=torch.rand(R, generator=g))


def inputs(family, N, Ne, R=R_CASE):
    inp = (grid_inputs if family == "grid" else random_inputs)(N, Ne, R)
    inp.update(upstream(R, N))
    return inp


def evaluate(inp, dtype, outer=lossfun_outer, distortion=lossfun_distortion):
    """The five outputs of a case through the given pair of functions on CPU tensors of `dtype` under autograd."""
    cv = lambda k: inp[k].to(dtype)
    with torch.enable_grad():
        w, we = cv("w").clone().requires_grad_(True), cv("w_env").clone().requires_grad_(True)
        loss = outer(cv("t"), w, cv("t_env"), we)
        g_w, g_we = torch.autograd.grad((loss * cv("up")).sum(), [w, we])
        dist = distortion(cv("t"), w)
        (g_dist,) = torch.autograd.grad((dist * cv("up_dist")).sum(), [w])
    return dict(loss=loss.detach(), g_w=g_w, g_w_env=g_we, dist=dist.detach(), g_dist=g_dist)


def checks(got, ref64, ref32=None, keys=OUTPUTS):
    return {k: worst_entry(got[k], ref64[k], DISTLOSS * scale_of(ref64[k]), ref32[k] if ref32 is not None else None) for k in keys}


@functools.lru_cache(maxsize=None)
def case(family, N, Ne, R=R_CASE):
    inp = inputs(family, N, Ne, R)
    return inp, evaluate(inp, torch.float64), evaluate(inp, torch.float32)


def _shape_of(key, N, Ne, R=R_CASE):
    return {"t": (R, N + 1), "w": (R, N), "t_env": (R, Ne + 1), "w_env": (R, Ne), "up": (R, N), "up_dist": (R,), "loss": (R, N),
            "g_w": (R, N), "g_w_env": (R, Ne), "dist": (R,), "g_dist": (R, N)}[key]


def fixture_case(g, family, N, Ne):
    """One case of tests/golden/g12_mip_losses.npz (g: the loaded fixture, name -> tensor): inputs, the reference's fp64 outputs and
    its fp32 outputs.  Every quantity is stored as one flat array per family, the cases in the order of FIXTURE_SHAPES; an fp32
    output is stored as its distance in units of the last place from the rounded fp64 output (tests/golden/make_mip_losses.py)."""
    def cut(name, key):
        flat = g[family + "/" + name]
        start = sum(int(torch.Size(_shape_of(key, n, ne)).numel()) for (n, ne) in FIXTURE_SHAPES[:FIXTURE_SHAPES.index((N, Ne))])
        shape = _shape_of(key, N, Ne)
        return flat[start:start + int(torch.Size(shape).numel())].reshape(shape)

    inp = {k: cut(k, k) for k in INPUTS}
    ref64 = {k: cut(k + "64", k) for k in OUTPUTS}
    ref32 = {k: (ref64[k].float().view(torch.int32) + cut(k + "32_ulps", k)).view(torch.float32) for k in OUTPUTS}
    return inp, ref64, ref32


def table():
    """(family, N, Ne) of the nine-row cases."""
    return [(f, n, ne) for f in FAMILIES for (n, ne) in SHAPES]


def case_id(family, N, Ne, R=R_CASE):
    return "%s_N%d_Ne%d" % (family, N, Ne) + ("" if R == R_CASE else "_R%d" % R)
