"""Case table, CPU restatement and per-entry bounds for the Mip-NeRF 360 extras (ops.mip_extras / training.mip_expected_distance over
neo_mip_extras / neo_mip_extras_backward): opacity, expected distance and distance percentiles of an interval histogram.  Plain CPU
torch, in the style of tests/mip_loss_cases.py: tests/test_mip_extras_cpu.py checks the restatement against the reference's own
integrate_weights / sorted_interp (tests/golden/g13_mip_extras.npz) and the condition of every case; tests/test_gpu_mip_extras.py
hands the same inputs to the kernels.

The restatement (mipnerf360/helper.py:168-172, :196-222, and the `compute_extras` slot of :264-274) is written for reading, not
speed: any dtype, differentiable; sorted_interp as a count of knots and two gathers, which on rows that do not decrease is
what the reference's masked maxima and minima select (the CPU test holds it to the reference's own results).

Shapes: n on the edges of a 64-lane round and of the entry points' limits at 9 rays, n = 64 repeated at the ray counts of
alongray_cases.RAY_COUNTS.  Quantiles: fp32 (0.05, 0.5, 0.95), and ONE case (grid, n = 65) with eight quantiles, 0 and 1 among them.
Two input families per shape:
  grid     edges = sorted integers out of 0 .. 4096 over 4096 (ties and zero-width intervals), weights = integers over 4096 with a
           quarter of them zero, sized so that a row sums to about 0.75; row 0 puts 1/2 on its first interval and nothing on the
           inner ones (the quantile 0.5 meets a run of tied knots exactly), row 1 sums to about 1.5 (the clip is active); upstream
           gradients in eighths.  Every prefix sum is exact in fp32 and fp64, so a quantile that lands exactly on a knot (0 and 1
           always do) takes the same branch everywhere;
  random   edges = sorted uniform sdist with the ends 0 and 1, weights = rand^3 normalised per row, and the degenerate rows
           0 all-zero weights, 1 one spike among weights of 1e-9, 2 a row summing to 1.7 (the clip at 1 is active), 3 a row summing
           to 0.3, 4 every second weight zero.
Each case runs under both edge conventions of the entry point: "sdist" - the edges are s in [0, 1], mapped with s_to_t for
near = 0.2, far = 3.0 (as fp32 scalars, which is what the entry point receives) - and "metric" - near = far = 0 and the edges are
distances already: the grid values themselves, or the fp32-rounded s_to_t of the random sdist.

Condition (checked over the whole table by the CPU test; it is not a tolerance): in the random family every quantile lies at least
KNOT_MARGIN = 1e-9 from every knot of the fp64 cumulative weight.  The percentile jumps where a quantile meets a knot at a zero-weight
interval, so the fp64 restatement and an fp64 scan in another summation order may only be compared where they cannot bracket a
quantile differently.

Bounds.  Every entry of every output, the gradient included, is within DISTLOSS x max(1, largest |fp64 value| of that tensor in the
case) of the fp64 restatement; DISTLOSS = 1e-6 is the constant the sibling along-ray kernels are held to.  No entry is exempted.
The reference's own fp32 arithmetic on the CPU is recorded next to every figure (worst_entry's fp32 column).  On this table it stays
inside the bound (worst entry: 0.41 of it, a percentile at n = 64; torch's CPU cumsum accumulates an fp32 row in a wider type, which
an fp32 scan on the device would not), so FP32_INSIDE lists every output.
"""
import functools

import numpy as np
import torch

from alongray_cases import DISTLOSS, RAY_COUNTS, assert_inside, scale_of, summarize, worst_entry  # noqa: F401

R_CASE = 9
NS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 1023, 1024)
FIXTURE_NS = tuple(n for n in NS if n <= 129)
MID_N = 64
FAMILIES = ("grid", "random")
CONVENTIONS = ("sdist", "metric")
NEAR, FAR = float(np.float32(0.2)), float(np.float32(3.0))       # the entry point takes fp32 scalars
U3 = (0.05, 0.5, 0.95)
U8 = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0)
U8_CASE = ("grid", 65)
KNOT_MARGIN = 1e-9
OUTPUTS = ("acc", "mean", "pct", "g_w")
FP32_INSIDE = OUTPUTS               # outputs on which the reference's fp32 arithmetic itself stays inside the bounds (module docstring)


def quantiles(u):
    return torch.tensor(u, dtype=torch.float32)


# ---- the reference's helpers, restated -------------------------------------------------------------------------------------------
def s_to_t(s, near=NEAR, far=FAR):
    """construct_ray_warps (helper.py:168-172): python-float s_near / s_far against a tensor of any dtype."""
    s_near, s_far = 1 / near, 1 / far
    return 1 / (s * s_far + (1 - s) * s_near)


def integrate_weights(w):
    """helper.py:196-203: the cumulative weight at every edge - 0, the running sum of all but the last weight cut off at 1, and 1.
    One knot per edge, no renormalisation."""
    inner = torch.cumsum(w[..., :-1], dim=-1).clamp(max=1.0)
    return torch.cat([torch.zeros_like(w[..., :1]), inner, torch.ones_like(w[..., :1])], dim=-1)


def sorted_interp(x, xp, fp):
    """helper.py:207-222 on rows that do not decrease: x (R, n_u), xp / fp (R, n + 1).  The reference masks with `x >= xp` and takes
    the largest masked and the smallest unmasked entry of xp and fp (the first / last entry when there is none).  On sorted rows the
    mask is a prefix of length c = #{j : xp_j <= x}, so these are the entries c - 1 and c, held inside the row.  The offset is
    clip(nan_to_num((x - xp0) / (xp1 - xp0), 0), 0, 1)."""
    last = xp.shape[-1] - 1
    c = (xp[..., :, None] <= x[..., None, :]).sum(-2)
    i0, i1 = torch.clamp(c - 1, min=0), torch.clamp(c, max=last)
    xp0, xp1 = torch.gather(xp, -1, i0), torch.gather(xp, -1, i1)
    fp0, fp1 = torch.gather(fp, -1, i0), torch.gather(fp, -1, i1)
    offset = torch.nan_to_num((x - xp0) / (xp1 - xp0), nan=0.0).clamp(0, 1)
    return fp0 + offset * (fp1 - fp0)


def acc_and_mean(t, w):
    """acc = sum w; distance_mean = clip(nan_to_num(sum w_i (t_i + t_{i+1}) / 2 / acc, nan=inf), t_0, t_n): t_n without weight."""
    acc = w.sum(-1)
    mean = (w * (t[..., 1:] + t[..., :-1]) / 2).sum(-1) / acc
    return acc, torch.clip(torch.nan_to_num(mean, nan=float("inf")), t[..., 0], t[..., -1])


def backward_formula(t, w, g_acc, g_mean):
    """The contract of neo_mip_extras_backward: g_w_i = g_acc + g_mean ((t_i + t_{i+1}) / 2 - mean) / acc, the second term 0 on a
    row with acc == 0 (autograd of acc_and_mean yields NaN there)."""
    acc = w.sum(-1, keepdim=True)
    mid = (t[..., 1:] + t[..., :-1]) / 2
    safe = torch.where(acc == 0, torch.ones_like(acc), acc)
    mean = (w * mid).sum(-1, keepdim=True) / safe
    second = g_mean[..., None] * (mid - mean) / safe
    return g_acc[..., None] + torch.where(acc == 0, torch.zeros_like(second), second)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _seed(n, R):
    return 13000 + n * 17 + (0 if R == R_CASE else 7919 * R)


def grid_inputs(n, R=R_CASE):
    g = torch.Generator().manual_seed(_seed(n, R))
    edges = torch.sort(torch.randint(0, 4097, (R, n + 1), generator=g), -1).values.float() / 4096
    hi = max(1, (2 * 4096) // n)
    w = torch.randint(0, hi + 1, (R, n), generator=g) * (torch.rand(R, n, generator=g) >= 0.25)
    if R > 0:                           # knots 0, 1/2, .., 1/2, 1: the quantile 0.5 meets a run of tied knots exactly
        w[0] = 0
        w[0, 0] = 2048
        w[0, n - 1] = 1024
    if R > 1:                           # the row passes 1: the clip is active
        w[1] = w[1] * 2 + 1
    return dict(edges=edges, w=w.float() / 4096)


def random_inputs(n, R=R_CASE):
    g = torch.Generator().manual_seed(_seed(n, R))
    edges = torch.sort(torch.rand(R, n + 1, generator=g), -1).values
    edges[:, 0], edges[:, -1] = 0, 1
    w = torch.rand(R, n, generator=g) ** 3
    w = w / w.sum(-1, keepdim=True)
    if R > 0:
        w[0] = 0.0
    if R > 1:
        w[1] = 1e-9
        w[1, n // 2] = 1.0
    if R > 2:
        w[2] = w[2] * 1.7
    if R > 3:
        w[3] = w[3] * 0.3
    if R > 4:
        w[4, 1::2] = 0.0
    return dict(edges=edges, w=w)


def upstream(R):
    g = torch.Generator().manual_seed(6)
    return dict(g_acc=(torch.randint(-8, 9, (R,), generator=g) / 8).float(), g_mean=(torch.randint(1, 9, (R,), generator=g) / 8).float())


def inputs(family, n, R=R_CASE):
    """edges: the family's raw values in [0, 1] (the "sdist" convention reads them as s)."""
    inp = (grid_inputs if family == "grid" else random_inputs)(n, R)
    inp.update(upstream(R))
    return inp


def kernel_edges(inp, family, convention):
    """(edges, near, far) as the entry point receives them under a convention."""
    if convention == "sdist":
        return inp["edges"], NEAR, FAR
    if family == "grid":
        return inp["edges"], 0.0, 0.0
    return s_to_t(inp["edges"].double()).float(), 0.0, 0.0


def evaluate(inp, family, convention, u, dtype, interp=sorted_interp, integrate=integrate_weights, warp=s_to_t):
    """The four outputs of a case on CPU tensors of `dtype` through the given helpers."""
    edges, near, _ = kernel_edges(inp, family, convention)
    t = edges.to(dtype)
    if near:
        t = warp(t)
    w = inp["w"].to(dtype)
    acc, mean = acc_and_mean(t, w)
    x = quantiles(u).to(dtype).expand(w.shape[0], len(u))
    pct = interp(x, integrate(w), t)
    return dict(acc=acc, mean=mean, pct=pct, g_w=backward_formula(t, w, inp["g_acc"].to(dtype), inp["g_mean"].to(dtype)))


def autograd_g_w(inp, family, convention):
    """fp64 autograd of acc_and_mean under the case's upstream gradients (NaN on a row without weight)."""
    edges, near, _ = kernel_edges(inp, family, convention)
    t = edges.double()
    if near:
        t = s_to_t(t)
    with torch.enable_grad():
        w = inp["w"].double().requires_grad_(True)
        acc, mean = acc_and_mean(t, w)
        (g,) = torch.autograd.grad((acc * inp["g_acc"].double() + mean * inp["g_mean"].double()).sum(), [w])
    return g


def knot_distance(inp, u):
    """Smallest |u_q - knot| over the quantiles and the fp64 knots of every row."""
    xp = integrate_weights(inp["w"].double())
    return float((quantiles(u).double()[None, None, :] - xp[..., None]).abs().min())


def checks(got, ref64, ref32=None, keys=OUTPUTS):
    return {k: worst_entry(got[k], ref64[k], DISTLOSS * scale_of(ref64[k]), ref32[k] if ref32 is not None else None) for k in keys}


@functools.lru_cache(maxsize=None)
def case(family, n, convention, R=R_CASE, u=U3):
    inp = inputs(family, n, R)
    return inp, evaluate(inp, family, convention, u, torch.float64), evaluate(inp, family, convention, u, torch.float32)


def table():
    """(family, n, convention, R, u) of every case: the nine-row shapes, the ray counts at n = 64 and the eight-quantile case."""
    rows = [(f, n, c, R_CASE, U3) for f in FAMILIES for n in NS for c in CONVENTIONS]
    rows += [(f, MID_N, c, r, U3) for f in FAMILIES for c in CONVENTIONS for r in RAY_COUNTS]
    rows += [U8_CASE + (c, R_CASE, U8) for c in CONVENTIONS]
    return rows


def case_id(family, n, convention, R=R_CASE, u=U3):
    return "%s_n%d_%s" % (family, n, convention) + ("" if R == R_CASE else "_R%d" % R) + ("" if u == U3 else "_u%d" % len(u))


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def fixture_cases():
    """(family, n, convention, u) of the cases tests/golden/g13_mip_extras.npz holds, in storage order."""
    rows = [(f, n, c, U3) for f in FAMILIES for n in FIXTURE_NS for c in CONVENTIONS]
    return rows + [U8_CASE + (c, U8) for c in CONVENTIONS]


def fixture_case(g, family, n, convention, u):
    """One case of the fixture (g: name -> tensor): inputs edges / w as stored, the reference's fp64 percentiles and its fp32 ones.
    Stored as flat arrays, the cases concatenated in the order of fixture_cases(); an fp32 result is stored as its distance in units
    of the last place from the rounded fp64 result (tests/golden/make_mip_extras.py)."""
    rows = fixture_cases()
    at = rows.index((family, n, convention, u))

    def cut(name, size_of):
        start = sum(size_of(r) for r in rows[:at])
        return g[name][start:start + size_of(rows[at])]

    edges = cut("edges", lambda r: R_CASE * (r[1] + 1)).reshape(R_CASE, n + 1)
    w = cut("w", lambda r: R_CASE * r[1]).reshape(R_CASE, n)
    pct64 = cut("pct64", lambda r: R_CASE * len(r[3])).reshape(R_CASE, len(u))
    ulps = cut("pct32_ulps", lambda r: R_CASE * len(r[3])).reshape(R_CASE, len(u))
    return dict(edges=edges, w=w), pct64, (pct64.float().view(torch.int32) + ulps).view(torch.float32)
