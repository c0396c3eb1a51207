"""Case table, fp64 CPU restatement and per-entry bounds for the NeO-360 extras (ops.tp_extras over neo_tp_extras, csrc/tp_extras.hip):
total opacity, expected disparity and distance percentiles of a ray's whole interval histogram, inside and outside the unit sphere
together, as distances along the ray.  Plain CPU torch, in the style of tests/mip_extras_cases.py: tests/test_tp_extras_cpu.py checks
the restatement in closed form and the condition of every case; tests/test_gpu_tp_extras.py hands the same inputs to the kernel.

The contract (include/neo360_hip.h).  Per ray, all inputs fp32, everything fp64 from them, each output rounded once:
  inside interval i   [fg_t[i], fg_t[i+1]], fg_t[N] := far, mass fg_w[i];
  outside interval j  in inverse radius [bg_s[j], bg_s[j+1]], bg_s[N] := 0, mass lambda bg_w[j]; the edge at inverse radius s lies at
                      tau(s) = d1 + sqrt(max(1 / s^2 - rho2, 0)) / |d|, d1 = -(o.d) / |d|^2, rho2 = |o + d1 d|^2, tau(0) = +inf;
  knots c_0 = 0, c_{k+1} = c_k + m_k (no renormalisation, no clamp); opacity = c_M; disparity = sum m_k (1 / a_k + 1 / b_k) / 2;
  pct(u) = +inf if u >= c_M, else with c_k <= u < c_{k+1}, off = (u - c_k) / m_k: inside a + off (b - a), outside
  tau(s_j + off (s_{j+1} - s_j)).  The inside-only form has the N inside intervals alone.

Shapes: N on the edges of a 64-lane round and the module's own sample counts (129, 385) up to the entry point's limit at 9 rays,
N = 64 repeated at the ray counts of alongray_cases.RAY_COUNTS; each shape in both forms ("two": two regions, "inside": inside only).
Quantiles: fp32 (0.05, 0.5, 0.95), and ONE case (grid, N = 65) with eight dyadic quantiles, 0 and 1 among them.

Rays: origins inside the unit sphere, directions NOT of unit length (|d| between 0.5 and 2).
  grid     every ray runs along a coordinate axis through the centre with a dyadic origin and |d| in {1/2, 2}: d1, far = tau(1) and
           tau(2^-e) are dyadic.  fg_t = far k / 4096 for sorted integers k in 1 .. 4096 (ties: zero-width intervals), bg_s = 2^-e for
           sorted integers e in 0 .. 12 starting at 0 (ties), lambda in {1/4, 1/2, 3/4}, weights = integers over 4096 with a quarter of
           them zero.  Every mass is a multiple of 2^-14 and every knot is exact in fp64 in ANY summation order, so a quantile that
           meets a knot takes the same bracket everywhere and the percentile there is the bracket's first edge exactly.  Row 0: mass
           1/2 on the first inside interval, then nothing up to the LAST outside interval - the median meets a run of tied knots
           that crosses the sphere (inside-only: the median is not below the opacity, +inf).  Row 1: mass 1/2 on the first inside
           interval, nothing up to the last inside one - the run stays inside.
  random   origins uniform in a ball of radius 0.8, directions uniform with |d| in [0.5, 2]; far = fp32(tau(1)); fg_t = far x sorted
           uniform in [0.02, 1]; bg_s = sorted uniform in [0.05, 1] descending, starting at 1; lambda uniform in [0.2, 0.8]; weights
           rand^3 with the inside row summing to 1 - lambda and the outside row to 1.  Degenerate rows: 0 all-zero weights; 1 lambda =
           0; 2 all mass in the last outside interval with bg_s[N-1] = 0 exactly (every percentile +inf, disparity 0); 3 bg_s[N-1] =
           2^-10, not exactly 0; 4 total mass 0.3 (upper percentiles +inf); 5 one spike among weights of 1e-9; 6 a ray through the
           centre (o = -d / 4 exactly: rho2 = 0); 7 bg_s[N-1] = 0 exactly with ordinary weights (the shape of the module's level-0 row).

Conditions (checked over the whole table by the CPU test; they are not tolerances): in the random family every quantile lies at least
KNOT_MARGIN = 1e-9 from every fp64 knot and from the total, so two fp64 scans in different summation orders cannot bracket a quantile
differently; and the restatement summed front to back agrees with the restatement summed pairwise within a tenth of the bound below
on every finite entry (with the same infinite entries).

Bounds.  Every finite entry of every output is within DISTLOSS x max(1, largest finite |fp64 value| of that tensor in the case) of the
fp64 restatement; DISTLOSS = 1e-6 is the constant the sibling along-ray kernels are held to.  Infinite entries match exactly.  No
entry is exempted.
"""
import functools

import torch

from alongray_cases import DISTLOSS, RAY_COUNTS, assert_inside, summarize, worst_entry  # noqa: F401

R_CASE = 9
NS = (1, 2, 3, 63, 64, 65, 129, 385, 1024)
MID_N = 64
FAMILIES = ("grid", "random")
FORMS = ("two", "inside")
U3 = (0.05, 0.5, 0.95)
U8 = (0.0, 0.0625, 0.25, 0.5, 0.75, 0.9375, 0.984375, 1.0)
U8_CASE = ("grid", 65)
KNOT_MARGIN = 1e-9
OUTPUTS = ("opacity", "disparity", "pct")
INF = float("inf")


def quantiles(u):
    return torch.tensor(u, dtype=torch.float32)


# ---- the contract, restated ------------------------------------------------------------------------------------------------------
def ray_geometry(o, d):
    """d1, rho2, |d| (R,) of rays o + t d: the parameter of the point nearest the centre, its squared radius, the direction's norm."""
    dd = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    d1 = -(o[:, 0] * d[:, 0] + o[:, 1] * d[:, 1] + o[:, 2] * d[:, 2]) / dd
    c = o + d1[:, None] * d
    rho2 = c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]
    return d1, rho2, torch.sqrt(dd)


def tau(s, geom):
    """Distance along the ray of the point at radius 1 / s: s (R, K) against per-ray geometry; tau(0) = +inf."""
    d1, rho2, dn = (g[:, None] for g in geom)
    safe = torch.where(s == 0, torch.ones_like(s), s)
    val = d1 + torch.sqrt(torch.clamp(1.0 / (safe * safe) - rho2, min=0.0)) / dn
    return torch.where(s == 0, torch.full_like(s, INF), val)


def prefix_sums(m, pairwise):
    """Inclusive prefix sums along the last axis: front to back (torch.cumsum), or by doubling strides (every prefix a balanced tree
    of partial sums - the order of a shuffle scan)."""
    if not pairwise:
        return torch.cumsum(m, dim=-1)
    c, o = m.clone(), 1
    while o < c.shape[-1]:
        c = torch.cat([c[..., :o], c[..., o:] + c[..., :-o]], dim=-1)
        o *= 2
    return c


def total_of(x, pairwise):
    """Sum along the last axis: front to back, or as a balanced tree."""
    if not pairwise:
        return prefix_sums(x, False)[..., -1]
    while x.shape[-1] > 1:
        if x.shape[-1] % 2:
            x = torch.cat([x, torch.zeros_like(x[..., :1])], dim=-1)
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def histogram(inp, form, dtype=torch.float64):
    """The M intervals of every ray in ray order: dict(m, e0, e1, a, b (R, M), outside (M,) bool, geom): masses, the interval ends in
    the region's own coordinate (t inside, inverse radius outside) and as distances, and which intervals are outside."""
    fg_t, fg_w, far = inp["fg_t"].to(dtype), inp["fg_w"].to(dtype), inp["far"].to(dtype)
    geom = ray_geometry(inp["rays_o"].to(dtype), inp["rays_d"].to(dtype))
    N = fg_t.shape[1]
    e0, e1 = fg_t, torch.cat([fg_t[:, 1:], far[:, None]], dim=-1)
    h = dict(m=fg_w, e0=e0, e1=e1, a=e0, b=e1, outside=torch.zeros(N, dtype=torch.bool), geom=geom)
    if form == "two":
        bg_s, bg_w, lam = inp["bg_s"].to(dtype), inp["bg_w"].to(dtype), inp["lam"].to(dtype)
        s0, s1 = bg_s, torch.cat([bg_s[:, 1:], torch.zeros_like(bg_s[:, :1])], dim=-1)
        h = dict(m=torch.cat([fg_w, lam[:, None] * bg_w], dim=-1), e0=torch.cat([e0, s0], dim=-1), e1=torch.cat([e1, s1], dim=-1),
                 a=torch.cat([e0, tau(s0, geom)], dim=-1), b=torch.cat([e1, tau(s1, geom)], dim=-1),
                 outside=torch.cat([h["outside"], torch.ones(N, dtype=torch.bool)]), geom=geom)
    return h


def knots(h, pairwise=False):
    """c_0 .. c_M (R, M + 1)."""
    return torch.cat([torch.zeros_like(h["m"][:, :1]), prefix_sums(h["m"], pairwise)], dim=-1)


def evaluate(inp, form, u, dtype=torch.float64, pairwise=False):
    """dict(opacity (R,), disparity (R,), pct (R, n_u), at_knot (R, n_u) bool: the quantile equals its bracket's first knot)."""
    h = histogram(inp, form, dtype)
    m, c = h["m"], knots(h, pairwise)
    R, M = m.shape
    x = quantiles(u).to(dtype).expand(R, len(u)).contiguous()
    k = torch.searchsorted(c[:, 1:].contiguous(), x, right=True)            # knots c_1 .. c_M at or below u: c_k <= u < c_{k+1}
    leaves = k >= M
    kk = torch.clamp(k, max=M - 1)
    take = lambda t: torch.gather(t, 1, kk)
    ck, mk = take(c[:, :-1]), take(m)
    off = (x - ck) / torch.where(leaves, torch.ones_like(mk), mk)
    inside = take(h["a"]) + off * (take(h["b"]) - take(h["a"]))
    outside = tau(take(h["e0"]) + off * (take(h["e1"]) - take(h["e0"])), h["geom"])
    pct = torch.where(h["outside"][kk], outside, inside)
    pct = torch.where(leaves, torch.full_like(pct, INF), pct)
    disparity = total_of(m * ((1.0 / h["a"] + 1.0 / h["b"]) * 0.5), pairwise)
    return dict(opacity=c[:, -1], disparity=disparity, pct=pct, at_knot=(x == ck) & ~leaves)


def knot_distance(inp, form, u):
    """Smallest |u_q - knot| over the quantiles and the fp64 knots of every row (the total is the last knot; c_0 = 0 is not one a
    quantile can be bracketed differently at)."""
    c = knots(histogram(inp, form))[:, 1:]
    return float((quantiles(u).double()[None, None, :] - c[..., None]).abs().min())


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _seed(n, R):
    return 41000 + n * 19 + (0 if R == R_CASE else 7919 * R)


_GRID_OX = (0.0, 0.25, -0.25, 0.5, -0.5, 0.125, -0.125, 0.375, -0.375)
_GRID_DX = (0.5, 2.0, -0.5, -2.0)
_GRID_LAM = (0.25, 0.5, 0.75)


def grid_inputs(n, R=R_CASE):
    g = torch.Generator().manual_seed(_seed(n, R))
    r = torch.arange(R)
    ox = torch.tensor(_GRID_OX)[r % 9]
    dx = torch.tensor(_GRID_DX)[r % 4]
    axis = r % 3
    rays_o, rays_d = torch.zeros(R, 3), torch.zeros(R, 3)
    rays_o[r, axis], rays_d[r, axis] = ox, dx
    far = -ox / dx + 1.0 / dx.abs()                             # d1 + 1 / |d|: dyadic
    k = torch.sort(torch.randint(1, 4097, (R, n), generator=g), -1).values
    fg_t = far[:, None] * (k.float() / 4096)
    e = torch.sort(torch.randint(0, 13, (R, n), generator=g), -1).values
    e[:, 0] = 0
    bg_s = torch.exp2(-e.float())
    hi = max(1, 4096 // n)
    fg_w = torch.randint(0, hi + 1, (R, n), generator=g) * (torch.rand(R, n, generator=g) >= 0.25)
    bg_w = torch.randint(0, 2 * hi + 1, (R, n), generator=g) * (torch.rand(R, n, generator=g) >= 0.25)
    if R > 0:                           # knots 0, 1/2, .., 1/2, 1/2 + lambda: the run of tied knots crosses the sphere
        fg_w[0], bg_w[0] = 0, 0
        fg_w[0, 0], bg_w[0, n - 1] = 2048, 4096
    if R > 1:                           # the run stays inside
        fg_w[1] = 0
        fg_w[1, n - 1] = 1024
        fg_w[1, 0] = 2048
    lam = torch.tensor(_GRID_LAM)[r % 3]
    return dict(rays_o=rays_o, rays_d=rays_d, far=far, fg_t=fg_t, fg_w=fg_w.float() / 4096, bg_s=bg_s, bg_w=bg_w.float() / 4096, lam=lam)


def random_inputs(n, R=R_CASE):
    g = torch.Generator().manual_seed(_seed(n, R))
    unit = lambda: torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    rays_o = unit() * (0.8 * torch.rand(R, 1, generator=g) ** (1 / 3))
    rays_d = unit() * (0.5 + 1.5 * torch.rand(R, 1, generator=g))
    if R > 6:
        rays_o[6] = -0.25 * rays_d[6]                           # through the centre: o + d / 4 = 0 exactly
    far = tau(torch.ones(R, 1, dtype=torch.float64), ray_geometry(rays_o.double(), rays_d.double()))[:, 0].float()
    fg_t = far[:, None] * torch.sort(0.02 + 0.98 * torch.rand(R, n, generator=g), -1).values
    bg_s = torch.sort(0.05 + 0.95 * torch.rand(R, n, generator=g), -1, descending=True).values
    bg_s[:, 0] = 1.0
    lam = 0.2 + 0.6 * torch.rand(R, generator=g)
    fg_w = torch.rand(R, n, generator=g) ** 3
    fg_w = fg_w / fg_w.sum(-1, keepdim=True) * (1.0 - lam[:, None])
    bg_w = torch.rand(R, n, generator=g) ** 3
    bg_w = bg_w / bg_w.sum(-1, keepdim=True)
    if R > 0:
        fg_w[0], bg_w[0] = 0.0, 0.0
    if R > 1:
        lam[1] = 0.0
        fg_w[1] = fg_w[1] / fg_w[1].sum() * 0.97
    if R > 2:
        fg_w[2], bg_w[2], lam[2] = 0.0, 0.0, 1.0
        bg_w[2, n - 1], bg_s[2, n - 1] = 1.0, 0.0
    if R > 3 and n > 1:
        bg_s[3, n - 1] = 2.0 ** -10
    if R > 4:
        fg_w[4], bg_w[4] = fg_w[4] * 0.3, bg_w[4] * 0.3
    if R > 5:
        fg_w[5], bg_w[5] = 1e-9, 1e-9
        fg_w[5, n // 2] = 1.0 - float(lam[5])
        bg_w[5, n // 2] = 1.0
    if R > 7 and n > 1:
        bg_s[7, n - 1] = 0.0
    return dict(rays_o=rays_o, rays_d=rays_d, far=far, fg_t=fg_t, fg_w=fg_w, bg_s=bg_s, bg_w=bg_w, lam=lam)


def inputs(family, n, R=R_CASE):
    return (grid_inputs if family == "grid" else random_inputs)(n, R)


def kernel_kwargs(inp, form, dev):
    """The arguments of ops.tp_extras for a case in a form, on a device."""
    kw = dict(fg_t=inp["fg_t"], fg_w=inp["fg_w"], far=inp["far"], rays_o=inp["rays_o"], rays_d=inp["rays_d"])
    if form == "two":
        kw.update(bg_s=inp["bg_s"], bg_w=inp["bg_w"], bg_lambda=inp["lam"])
    return {k: v.to(dev) for k, v in kw.items()}


# ---- comparing -------------------------------------------------------------------------------------------------------------------
def finite_scale(ref64):
    """max(1, largest finite |fp64 value|) of a tensor (1 when it has no finite entry)."""
    fin = ref64[torch.isfinite(ref64)]
    return max(1.0, float(fin.abs().max())) if fin.numel() else 1.0


def check_output(got, ref64, label, share=1.0):
    """Infinite entries of the reference match exactly; every finite one is inside share x DISTLOSS x finite_scale.  Returns the
    worst_entry record of the finite part."""
    got = torch.as_tensor(got).detach().cpu().double()
    assert got.shape == ref64.shape, (label, tuple(got.shape), tuple(ref64.shape))
    inf = torch.isinf(ref64)
    assert torch.equal(got[inf], ref64[inf]), (label, "an entry that must be +inf is not", got[inf], ref64[inf])
    assert not bool(torch.isnan(ref64).any()), (label, "NaN in the reference")
    return worst_entry(got[~inf], ref64[~inf], share * DISTLOSS * finite_scale(ref64))


def checks(got, ref64, label, share=1.0):
    return {k: check_output(got[k], ref64[k], (label, k), share) for k in OUTPUTS}


@functools.lru_cache(maxsize=None)
def case(family, n, form, R=R_CASE, u=U3):
    inp = inputs(family, n, R)
    return inp, evaluate(inp, form, u)


def table():
    """(family, n, form, R, u) of every case: the nine-row shapes, the ray counts at N = 64 and the eight-quantile case."""
    rows = [(f, n, m, R_CASE, U3) for f in FAMILIES for n in NS for m in FORMS]
    rows += [(f, MID_N, m, r, U3) for f in FAMILIES for m in FORMS for r in RAY_COUNTS]
    rows += [U8_CASE + (m, R_CASE, U8) for m in FORMS]
    return rows


def case_id(family, n, form, R=R_CASE, u=U3):
    return "%s_n%d_%s" % (family, n, form) + ("" if R == R_CASE else "_R%d" % R) + ("" if u == U3 else "_u%d" % len(u))
