"""Case table and per-entry bounds for the wave-per-ray kernels (compositing and its backward, distortion loss, the two
inverse-CDF resamplers, the Mip-NeRF 360 resampler and compositing pair).  Plain CPU torch: tests/test_alongray_cases_cpu.py
checks the conditions of every case (finite fp64 references, the fp32 oracle inside the bounds) on the very inputs that
tests/test_gpu_alongray_sweep.py hands to the kernels.

Sample counts sit on the edges of a 64-lane round (1, 2, 63, 64, 65, ...) and of the entry points' limits; every (kernel, N)
case has R = 9 rays whose first rows are degenerate (listed at each builder), and one mid-sized N per kernel is repeated at
R in RAY_COUNTS with ordinary rows, so that blocks of four waves with one, two and three idle waves occur.

Bounds.  The constants are those of the single-shape tests that existed before (test_gpu_training.py, test_gpu_stages.py,
test_gpu_mip_training.py); what they are relative to is decided here, entry by entry:
  outputs     constant x max(1, largest |fp64 value| of that output in the case);
  gradients   the last sample of compositing modes 0 and 2 has the interval 1e10 (a SENTINEL entry: its density gradient is
              1e10 G T and dwarfs every other entry of the tensor).  Non-sentinel entries: constant x max(1, largest |fp64
              gradient| among the non-sentinel entries).  A sentinel entry: constant x max(1, |its own fp64 gradient|) + 3 x
              its own |fp32 oracle - fp64 oracle| (behind nearly opaque material the sentinel multiplies the absolute rounding
              of the fp32 transmittance by 1e10: two correct evaluations of the same formula differ; conftest's standing rule
              for such entries is tol + 3 noise).  MAX_LIFTED_RAYS caps how many rays of a case may need that term.
"""
import functools

import numpy as np
import torch

import cases
import oracle
from neo360_amd import synth
from oracle import mip360
from oracle import training as T

# ---- the constants of the earlier single-shape tests -------------------------------------------------------------------------
OUT = 2e-6            # composited outputs (test_gpu_training.py, test_gpu_stages.py::test_composite_modes)
G_RGB = 2e-6          # colour gradient of the compositing backward
G_SIGMA = 2e-5        # density gradient of the compositing backward
DISTLOSS = 1e-6       # distortion loss and its gradient
LOOKUP = 1e-5         # feature lookups forward and backward
CDF = 2e-6            # resampled positions in cdf space
POS = 5e-6            # resampled positions on well-conditioned ascending rows
DESC = 1e-4           # descending rows: 1e-4, or 1e-4 + 3 x the row's fp32-vs-fp64 disagreement
MIP_S = 2e-5          # Mip-NeRF 360 interval endpoints
MIP_W, MIP_C, MIP_G = 2e-6, 5e-6, 2e-5      # Mip-NeRF 360 compositing: weights, colour, gradients
MAX_LIFTED_RAYS = 1   # rays of a nine-row case whose sentinel bound the noise term may lift (the spike row)

R_DEG = 9             # rays of a (kernel, N) case; rows 0 .. are the degenerate ones
RAY_COUNTS = (1, 2, 3, 5, 7, 201)                     # 201 = 4 * 50 + 1
EDGE_N = (1, 2, 3, 63, 64, 65, 127, 128, 129, 385, 1023, 1024)
COMPOSITE_N = EDGE_N
COMPOSITE_MODES = (0, 1, 2)
COMPOSITE_MID_N = 129
DISTLOSS_N = EDGE_N
DISTLOSS_MID_N = 385
# (n_prev, n_new): n_prev 4 (smallest) .. 257 (largest); n_prev + n_new = 256 / 257 / 512 / 513 / 1024: the three sort widths
# (256, 512, 1024 entries of LDS) at their lower and upper edges
RESAMPLE_SHAPES = ((4, 252), (64, 192), (66, 191), (65, 447), (66, 447), (129, 895), (257, 767))
RESAMPLE_MID = (65, 128)
MIP_RESAMPLE_N = (2, 63, 64, 65, 256)
MIP_RESAMPLE_NPREV = {True: (2, 24, 64, 85), False: (1, 2, 64, 65, 255)}      # dilated: 3 * 85 + 1 = 256 points
MIP_RESAMPLE_MID = (24, 32, True)
MIP_COMPOSITE_N = (1, 2, 63, 64, 65, 129, 256)
MIP_COMPOSITE_MID_N = 65
MIP_NEAR, MIP_FAR, MIP_DILATION, MIP_ANNEAL = 0.2, 3.0, 0.01, 0.7
EPS32 = float(torch.finfo(torch.float32).eps)


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)))


def _d(x):
    return x.detach()


# ---- comparing entry by entry --------------------------------------------------------------------------------------------------
def scale_of(ref64):
    """max(1, largest |fp64 value|) of a tensor (1 for an empty one)."""
    return max(1.0, float(ref64.abs().max())) if ref64.numel() else 1.0


def worst_entry(got, ref64, bound, ref32=None):
    """The entry of `got` that uses most of its bound: dict(err, bound, ratio, fp32) with fp32 = the fp32 oracle's own error at
    ITS worst entry under the same bounds.  bound: a float or a tensor of ref64's shape."""
    got = torch.as_tensor(got).detach().cpu().double()
    ref64 = ref64.double()
    assert got.shape == ref64.shape, (tuple(got.shape), tuple(ref64.shape))
    if got.numel() == 0:
        return dict(err=0.0, bound=float(torch.as_tensor(bound).max()), ratio=0.0, fp32=0.0, fp32_ratio=0.0)
    assert bool(torch.isfinite(got).all()), "non-finite result"
    bound = torch.broadcast_to(torch.as_tensor(bound, dtype=torch.float64), ref64.shape)
    err = (got - ref64).abs()
    ratio = (err / bound).reshape(-1)
    i = int(ratio.argmax())
    out = dict(err=float(err.reshape(-1)[i]), bound=float(bound.reshape(-1)[i]), ratio=float(ratio[i]), fp32=0.0, fp32_ratio=0.0)
    if ref32 is not None:
        e32 = (ref32.double() - ref64).abs()
        r32 = (e32 / bound).reshape(-1)
        j = int(r32.argmax())
        out.update(fp32=float(e32.reshape(-1)[j]), fp32_ratio=float(r32[j]))
    return out


def summarize(checks):
    """{quantity: worst_entry(...)} -> the compact record of one case for the parity report: per quantity [error, its bound, the
    fp32 oracle's error], and the largest share of a bound used."""
    rec = {k: [float("%.3g" % v["err"]), float("%.3g" % v["bound"]), float("%.3g" % v["fp32"])] for k, v in checks.items()}
    rec["worst_share_of_bound"] = float("%.3g" % max(v["ratio"] for v in checks.values()))
    rec["fp32_oracle_worst_share"] = float("%.3g" % max(v["fp32_ratio"] for v in checks.values()))
    return rec


def assert_inside(checks, label):
    for k, v in checks.items():
        assert v["ratio"] <= 1.0, (label, k, "error %.3e over its bound %.3e (fp32 oracle: %.3e)" % (v["err"], v["bound"], v["fp32"]))


# ---- compositing ---------------------------------------------------------------------------------------------------------------
def composite_deltas(mode, t, dirs, far):
    """fp64 interval of every sample as the three modes define it (oracle.compositing)."""
    t = t.double()
    if mode == 2:
        return torch.cat([t[:, :-1] - t[:, 1:], torch.full_like(t[:, :1], 1e10)], dim=-1)
    last = far.double() - t[:, -1:] if mode == 1 else torch.full_like(t[:, :1], 1e10)
    return torch.cat([t[:, 1:] - t[:, :-1], last], dim=-1) * dirs.double().norm(dim=-1, keepdim=True)


def composite_upstream(R, N, seed=11):
    """Upstream gradients of (rgb, acc, weights, bg_lambda, depth), drawn as test_composite_backward_matches_autograd always has."""
    gen = torch.Generator().manual_seed(seed)
    return dict(rgb=torch.randn(R, 3, generator=gen), acc=torch.randn(R, generator=gen), weights=torch.randn(R, N, generator=gen) * 0.1,
                lam=torch.randn(R, 1, generator=gen), depth=torch.randn(R, generator=gen))


def composite_inputs(mode, N, R=R_DEG, degenerate=True):
    """rgb (R,N,3), sigma (R,N,1), t (R,N), dirs (R,3), far (R,1), up.  Mode 0: |dirs| = 1.3; mode 2: t is the descending inverse
    radius.  Degenerate rows (R >= 9): 0 all-zero density; 1 opaque at the first sample (sigma 1e4); 2 one spike of optical depth
    15.5 in an otherwise empty ray (transmittance 1.9e-7 behind it: the sentinel entry of this row is the one the fp32 and fp64
    oracles disagree on); 3 a repeated position (one interval of width 0); 4 density 1e-6 throughout (N <= 129; an ordinary row
    above: fp32's 1 - exp(-sigma delta) carries an absolute rounding of 3e-8 per sample, which on a thin ray - transmittance ~1
    along all of it - adds up with N until the reference's own arithmetic misses the output bound; fp32 oracle, density 1e-6 at
    N = 385 in mode 1: acc 3.8e-6 against 2e-6; density 1e-3 at N = 1024 in mode 0: weights 2.7e-6 against 2e-6); 5 a ramp that
    saturates (sigma up to 400); 6 a last sample with sigma 1.3e-9 (sigma x 1e10 between transparent and opaque); the
    rest ordinary."""
    tag = "ar_comp_%d_%d_%d/" % (mode, N, R)
    rgb = synth.uniform(21, tag + "rgb", (R, N, 3), 0.0, 1.0)
    sigma = synth.uniform(21, tag + "sig", (R, N, 1), 0.0, 6.0)
    t = torch.cumsum(synth.uniform(21, tag + "t", (R, N), 0.002, 0.03), dim=-1)
    dirs = torch.nn.functional.normalize(synth.uniform(21, tag + "d", (R, 3), -1.0, 1.0), dim=-1) * (1.3 if mode == 0 else 1.0)
    far = t[:, -1:] + 0.02
    if mode == 2:
        t = torch.flip(t / t.max(), dims=[-1]).contiguous()
    k = (N - 1) // 2
    if degenerate and R >= R_DEG:
        if N >= 2:
            t[3, k + 1] = t[3, k]
        sigma[0] = 0.0
        sigma[1, 0] = 1e4
        sigma[2] = 0.0
        sigma[2, k] = float(15.5 / composite_deltas(mode, t, dirs, far)[2, k])
        if N <= 129:
            sigma[4] = 1e-6
        sigma[5, :, 0] = torch.linspace(0.0, 400.0, N) if N > 1 else torch.tensor([400.0])
        sigma[6, -1] = 1.3e-9
    return dict(rgb=rgb, sigma=sigma, t=t, dirs=dirs, far=far, up=composite_upstream(R, N, 11 + N))


def legacy_composite_inputs(mode):
    """The inputs test_gpu_training.py::test_composite_backward_matches_autograd has always used: cases.composite_case() (64 rays x
    129 samples, ray 0 empty, ray 1 sigma 80), mode 0 with |dirs| = 1.3, mode 2 on the flipped normalised t."""
    rgb, sigma, t, dirs, far = cases.composite_case()
    if mode == 2:
        t = torch.flip(t / t.max(), dims=[-1]).contiguous()
    if mode == 0:
        dirs = dirs * 1.3
    return dict(rgb=rgb, sigma=sigma, t=t, dirs=dirs, far=far, up=composite_upstream(64, 129, 11))


COMPOSITE_OUTPUTS = ("rgb", "acc", "weights", "depth", "lam")


def composite_oracle(inp, mode, white, dtype, which=None):
    """Outputs and the gradients of loss = sum over the outputs in `which` (default: all the mode has) of (output x its upstream
    gradient) with respect to rgb and sigma, through oracle.compositing under autograd in `dtype`."""
    c = lambda x: x.to(dtype)
    with torch.enable_grad():
        rc, sc = c(inp["rgb"]).clone().requires_grad_(True), c(inp["sigma"]).clone().requires_grad_(True)
        if mode == 0:
            rgb, acc, w, depth = oracle.compositing.vanilla_composite(rc, sc, c(inp["t"]), c(inp["dirs"]), white)
            lam = None
        else:
            rgb, acc, w, lam, depth = oracle.compositing.neo_composite(rc, sc, c(inp["t"]), c(inp["dirs"]), mode == 1,
                                                                       c(inp["far"]) if mode == 1 else None, white)
        outs = dict(rgb=rgb, acc=acc, weights=w, depth=depth)
        if mode == 1:
            outs["lam"] = lam
        names = [k for k in COMPOSITE_OUTPUTS if k in outs and (which is None or k in which)]
        loss = sum((outs[k] * c(inp["up"][k])).sum() for k in names)
        g_rgb, g_sigma = torch.autograd.grad(loss, [rc, sc], allow_unused=True)
    res = {k: _d(v) for k, v in outs.items()}
    res.update(g_rgb=torch.zeros_like(rc) if g_rgb is None else g_rgb, g_sigma=g_sigma[..., 0])
    return res


def sentinel_mask(mode, R, N):
    """(R,N) bool: the entries whose interval is the 1e10 sentinel (the last sample in modes 0 and 2)."""
    m = torch.zeros(R, N, dtype=torch.bool)
    if mode != 1:
        m[:, -1] = True
    return m


def sigma_grad_bounds(mode, g64, g32):
    """Per-entry bound (R,N) of the density gradient and the (R,) mask of the rays whose sentinel bound the noise term lifts to more
    than twice the plain constant x max(1, |own fp64 gradient|)."""
    sent = sentinel_mask(mode, *g64.shape)
    g64 = g64.double()
    rest = g64[~sent]
    bound = torch.full(g64.shape, G_SIGMA * scale_of(rest), dtype=torch.float64)
    plain = G_SIGMA * g64.abs().clamp(min=1.0)
    noise = 3.0 * (g32.double() - g64).abs()
    bound = torch.where(sent, plain + noise, bound)
    lifted = (sent & (noise > plain)).any(dim=-1)
    return bound, lifted


def old_sigma_grad_check(err, g64):
    """The expression the compositing-backward test used before: one bound for the whole tensor, scaled by its largest entry."""
    return float(err.abs().max()) < 2e-5 * max(1.0, float(g64.abs().max()))


def sigma_grad_inside(got, mode, g64, g32):
    bound, _ = sigma_grad_bounds(mode, g64, g32)
    return bool(((torch.as_tensor(got).double() - g64.double()).abs() <= bound).all())


def composite_checks(got, mode, ref64, ref32):
    """got: dict of the wrapper's outputs / gradients under the names of composite_oracle (a subset is fine) -> {name: worst_entry}."""
    checks = {}
    for k in COMPOSITE_OUTPUTS:
        if k in got and k in ref64:
            checks[k] = worst_entry(got[k], ref64[k], OUT * scale_of(ref64[k]), ref32[k])
    if "g_rgb" in got:
        checks["g_rgb"] = worst_entry(got["g_rgb"], ref64["g_rgb"], G_RGB * scale_of(ref64["g_rgb"]), ref32["g_rgb"])
    if "g_sigma" in got:
        bound, _ = sigma_grad_bounds(mode, ref64["g_sigma"], ref32["g_sigma"])
        checks["g_sigma"] = worst_entry(got["g_sigma"], ref64["g_sigma"], bound, ref32["g_sigma"])
    return checks


@functools.lru_cache(maxsize=None)
def composite_case(mode, N, white, R=R_DEG, degenerate=True, which=None, legacy=False):
    """(inputs, fp64 reference, fp32 reference) of one case, computed once per session."""
    inp = legacy_composite_inputs(mode) if legacy else composite_inputs(mode, N, R, degenerate)
    return inp, composite_oracle(inp, mode, white, torch.float64, which), composite_oracle(inp, mode, white, torch.float32, which)


def composite_table():
    """(mode, N, white) of the nine-row cases."""
    return [(m, n, w) for m in COMPOSITE_MODES for n in COMPOSITE_N for w in (False, True)]


# ---- distortion loss -----------------------------------------------------------------------------------------------------------
def distloss_inputs(N, R=R_DEG, degenerate=True):
    """w (R,N) weights of total 0.2 .. 1, m (R,N) ascending midpoints in (0,1), interval 1/N.  Degenerate rows: 0 all-zero weights;
    1 one non-zero weight; 2 all midpoints equal."""
    gen = _gen(23, N, R)
    w = torch.rand(R, N, generator=gen)
    w = w / w.sum(-1, keepdim=True) * (0.2 + 0.8 * torch.rand(R, 1, generator=gen))
    m = torch.sort(torch.rand(R, N, generator=gen), dim=-1).values
    if degenerate and R >= R_DEG:
        w[0] = 0.0
        w[1] = 0.0
        w[1, N // 2] = 0.7
        m[2] = 0.37
    return dict(w=w, m=m, interval=1.0 / N)


def distloss_oracle(inp, dtype):
    with torch.enable_grad():
        w = inp["w"].to(dtype).clone().requires_grad_(True)
        loss = T.eff_distloss(w, inp["m"].to(dtype), inp["interval"])
        (g,) = torch.autograd.grad(loss * 3.0, w)
    return dict(loss=_d(loss).reshape(1), g_w=g)


def distloss_checks(got, ref64, ref32):
    return dict(loss=worst_entry(got["loss"], ref64["loss"], DISTLOSS * scale_of(ref64["loss"]), ref32["loss"]),
                g_w=worst_entry(got["g_w"], ref64["g_w"], DISTLOSS * scale_of(ref64["g_w"]), ref32["g_w"]))


@functools.lru_cache(maxsize=None)
def distloss_case(N, R=R_DEG, degenerate=True):
    inp = distloss_inputs(N, R, degenerate)
    return inp, distloss_oracle(inp, torch.float64), distloss_oracle(inp, torch.float32)


# ---- inverse-CDF resampling (neo_resample / neo_resample_u) ------------------------------------------------------------------------
RESAMPLE_WELL_FROM = 4          # rows 4 .. of a nine-row case have weights in [0.25, 1]


def resample_inputs(n_prev, n_new, R=R_DEG, degenerate=True):
    """ASCENDING t_prev (R,n_prev) in (0,1], weights (R,n_prev) in [0.25,1], the deterministic quantile row u_det (n_new,) and the
    (seed, stream) of the randomized draws.  Degenerate rows: 0 all-zero weights (uniform fallback); 1 one spike (in a wide bin); 2 weights spanning
    1e-8 .. 1 (on bins of even width); 3 two equal consecutive bin edges (three equal previous samples); rows 4 .. are well conditioned.  A descending case
    is this one with t_prev flipped (the background branch: same weights, the bins scanned in the other order)."""
    tag = "ar_rs_%d_%d_%d/" % (n_prev, n_new, R)
    inc = synth.uniform(27, tag + "t", (R, n_prev), 0.01, 1.0)
    w = synth.uniform(27, tag + "w", (R, n_prev), 0.25, 1.0)
    k = n_prev // 2
    if degenerate and R >= R_DEG:
        # cdf space is only as good as fp32 positions x the slope of the cdf (pdf / bin width): the spike sits in a bin a quarter of
        # the range wide, and the wide-range weights on bins of even width (at n_prev = 257 a spike in an ordinary bin has slope 257
        # and a half-ulp of the position is 8e-6 of cdf, in the reference's own fp32 run too)
        inc[1, k] = inc[1, k + 1] = 0.0
        inc[1, k] = inc[1, k + 1] = 0.5 * float(inc[1].sum())
        inc[2] = 0.5 + 0.5 * inc[2]
    t_prev = torch.cumsum(inc, dim=-1)
    t_prev = t_prev / t_prev[:, -1:]
    if degenerate and R >= R_DEG:
        w[0] = 0.0
        w[1] = 0.0
        w[1, k] = 3.0
        w[2] = 10.0 ** synth.uniform(27, tag + "w2", (n_prev,), -8.0, 0.0)
        j = min(k, n_prev - 3)
        t_prev[3, j + 1] = t_prev[3, j]
        t_prev[3, j + 2] = t_prev[3, j]
    u_det = torch.linspace(0.0, 1.0 - 2 ** -32, n_new)             # the sampler's own fp32 table (helper.py:195)
    return dict(t_prev=t_prev.contiguous(), w=w, u_det=u_det, seed=4242 + n_prev, stream=5)


def resample_oracle(t_prev, w, u, dtype):
    """Merged, ASCENDING positions (R, n_prev + n_new) of the pinned oracle in `dtype`; u (n_new,) or (R, n_new) fp32 quantiles, the
    same numbers in either arithmetic.  t_prev may ascend or descend."""
    tp = t_prev.to(dtype)
    mids = 0.5 * (tp[..., 1:] + tp[..., :-1])
    uu = torch.broadcast_to(u.to(dtype), (tp.shape[0], u.shape[-1]))
    new = oracle.sampling.piecewise_constant_samples(mids, w[..., 1:-1].to(dtype), uu.shape[-1], u=uu)
    return oracle.sampling.merge_sorted(tp, new)


def cdf_space(x, bins, w_inner):
    """Evaluate the piecewise-linear CDF the sampler inverts (fp64) at positions x.
    Sample POSITIONS are ill-conditioned where the density is ~0 (an ulp of the
    cdf moves them by ulp/density), their CDF VALUES are not: stage parity of the
    resampler is asserted in cdf space, plus in position space on well-conditioned rows."""
    w = w_inner.double()
    tot = w.sum(-1, keepdim=True)
    pad = torch.clamp(1e-5 - tot, min=0)
    w = w + pad / w.shape[-1]
    pdf = w / (tot + pad)
    cdf = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf[:, :-1], -1).clamp(max=1), torch.ones_like(pdf[:, :1])], -1)
    b = bins.double()
    out = torch.empty_like(x, dtype=torch.float64)
    for r in range(x.shape[0]):
        out[r] = torch.from_numpy(np.interp(x[r].double().numpy(), b[r].numpy(), cdf[r].numpy()))
    return out


def resample_invariants(got, t_prev, n_new, descending):
    """What holds exactly whatever the arithmetic: the length, the order, and the previous samples present bit for bit."""
    got, t_prev = torch.as_tensor(got).detach().cpu(), t_prev.cpu()
    assert got.shape == (t_prev.shape[0], t_prev.shape[1] + n_new), tuple(got.shape)
    assert bool(torch.isfinite(got).all())
    asc = torch.flip(got, dims=[-1]) if descending else got
    assert bool((asc[:, 1:] >= asc[:, :-1]).all()), "output not sorted"
    for r in range(got.shape[0]):
        vals, counts = torch.unique(t_prev[r], return_counts=True)
        have = (got[r][None, :] == vals[:, None]).sum(dim=-1)
        assert bool((have >= counts).all()), ("previous samples missing from row", r)


def resample_checks(got, inp, u, descending, ref64, ref32, well_from=RESAMPLE_WELL_FROM):
    """got (R, n_out) as the wrapper returns it.  Ascending: cdf space on every sample (CDF) and positions on the well-conditioned
    rows (POS), fp64 oracle as truth.  Descending: the per-row rule of test_resample_matches_oracle around the fp32 oracle - 1e-4 +
    3 x the row's own fp32-vs-fp64 disagreement, which is plain 1e-4 on every row the reference determines to better than 1e-5."""
    got = torch.as_tensor(got).detach().cpu()
    if not descending:
        mids = 0.5 * (inp["t_prev"][:, 1:] + inp["t_prev"][:, :-1])
        wi = inp["w"][:, 1:-1]
        c64 = cdf_space(ref64, mids, wi)
        checks = dict(cdf=worst_entry(cdf_space(got, mids, wi), c64, CDF, cdf_space(ref32, mids, wi)))
        if got.shape[0] > well_from:
            checks["pos"] = worst_entry(got[well_from:], ref64[well_from:], POS, ref32[well_from:])
        return checks
    asc = torch.flip(got, dims=[-1])
    noise = (ref32.double() - ref64).abs().amax(dim=-1, keepdim=True)
    bound = torch.where(noise < 1e-5, torch.full_like(noise, DESC), DESC + 3.0 * noise)
    return dict(pos_desc=worst_entry(asc, ref32.double(), torch.broadcast_to(bound, ref64.shape), None))


def descending_well_determined(ref64, ref32):
    """(R,) bool: rows of a descending case the reference's own arithmetic determines to better than 1e-5."""
    return (ref32.double() - ref64).abs().amax(dim=-1) < 1e-5


@functools.lru_cache(maxsize=None)
def resample_case(n_prev, n_new, descending, R=R_DEG, degenerate=True):
    """(inputs with t_prev in the case's order, fp64 reference, fp32 reference) for the deterministic quantiles."""
    inp = dict(resample_inputs(n_prev, n_new, R, degenerate))
    if descending:
        inp["t_prev"] = torch.flip(inp["t_prev"], dims=[-1]).contiguous()
    return (inp, resample_oracle(inp["t_prev"], inp["w"], inp["u_det"], torch.float64),
            resample_oracle(inp["t_prev"], inp["w"], inp["u_det"], torch.float32))


def resample_draws(inp, R, n_new):
    """The randomized draws of a case as the device generator produces them (oracle.training.philox_uniform is bit-exact to it)."""
    return T.philox_uniform(inp["seed"], inp["stream"], R, n_new)


# ---- Mip-NeRF 360 proposal resampling ----------------------------------------------------------------------------------------------
def mip_resample_inputs(n_prev, n, dilate, R=R_DEG, degenerate=True):
    """s_prev (R,n_prev+1) from 0 to 1, w_prev (R,n_prev) normalised, the deterministic and the randomized quantile tables and one
    jitter per ray.  Degenerate rows: 0 a zero-width interval (logit -inf); 1 one dominant weight."""
    gen = _gen(27, n_prev, n, int(dilate), R)
    s_prev = torch.sort(torch.rand(R, n_prev + 1, generator=gen), dim=-1).values
    s_prev[:, 0], s_prev[:, -1] = 0.0, 1.0
    w_prev = torch.rand(R, n_prev, generator=gen) ** 3 + 1e-4
    k = n_prev // 2
    if degenerate and R >= R_DEG and n_prev >= 2:
        s_prev[0, k] = s_prev[0, k + 1]                          # interval k of row 0 has width 0
        w_prev[1] = 0.03 / n_prev
        w_prev[1, k] = 0.97
    w_prev = w_prev / w_prev.sum(-1, keepdim=True)
    u_max = EPS32 + (1 - EPS32) / n
    max_jitter = (1 - u_max) / (n - 1) - EPS32
    pad = 1 / (2 * n)
    return dict(s_prev=s_prev, w_prev=w_prev, jitter=torch.rand(R, 1, generator=gen) * max_jitter,
                u_rand=torch.linspace(0, 1 - u_max, n), u_det=torch.linspace(pad, 1 - pad - EPS32, n))


def mip_resample_oracle(inp, n, dilate, randomized, dtype):
    t, w = inp["s_prev"].to(dtype), inp["w_prev"].to(dtype)
    if dilate:
        t, w = mip360.max_dilate_weights(t, w, MIP_DILATION, (0.0, 1.0))
        t, w = t[..., 1:-1], w[..., 1:-1]
    logits = torch.where(t[..., 1:] > t[..., :-1], MIP_ANNEAL * torch.log(w), torch.full_like(w, -torch.inf))
    return mip360.sample_intervals(t, logits, n, (0.0, 1.0), inp["jitter"].to(dtype) if randomized else None)


def mip_tdist_of(sdist):
    """construct_ray_warps (helper.py:171-175) in fp32 on given interval endpoints."""
    s_near, s_far = np.float32(1.0 / MIP_NEAR), np.float32(1.0 / MIP_FAR)
    return 1.0 / (sdist * float(s_far) + (1.0 - sdist) * float(s_near))


def mip_resample_checks(sdist, tdist, ref64, ref32):
    sdist, tdist = torch.as_tensor(sdist).detach().cpu(), torch.as_tensor(tdist).detach().cpu()
    assert bool((sdist[:, 1:] >= sdist[:, :-1]).all()), "interval endpoints not sorted"
    want_t = mip_tdist_of(sdist).double()
    # four fp32 operations on the kernel's own endpoints: a relative 1e-6 is 8 ulp
    return dict(sdist=worst_entry(sdist, ref64, MIP_S, ref32), tdist_of_own_sdist=worst_entry(tdist, want_t, 1e-6 * want_t.abs(), None))


@functools.lru_cache(maxsize=None)
def mip_resample_case(n_prev, n, dilate, randomized, R=R_DEG, degenerate=True):
    inp = mip_resample_inputs(n_prev, n, dilate, R, degenerate)
    return (inp, mip_resample_oracle(inp, n, dilate, randomized, torch.float64),
            mip_resample_oracle(inp, n, dilate, randomized, torch.float32))


def mip_resample_table():
    return [(p, n, d) for d in (True, False) for p in MIP_RESAMPLE_NPREV[d] for n in MIP_RESAMPLE_N]


# ---- Mip-NeRF 360 compositing ------------------------------------------------------------------------------------------------------
def mip_composite_inputs(n, R=R_DEG, degenerate=True):
    """rgb (R,n,3), density (R,n), tdist (R,n+1) ascending in (0.2, 4.2), dirs (R,3), upstream gradients of weights and colour.
    Degenerate rows: 0 and 5 thin (the background term is active); 1 an opaque first interval; 2 zero density; 3 a ramp that
    saturates (density up to 400); 4 a zero-width interval."""
    gen = _gen(29, n, R)
    rgb = torch.rand(R, n, 3, generator=gen)
    dens = torch.rand(R, n, generator=gen) * 4.0
    t = torch.sort(torch.rand(R, n + 1, generator=gen) * 4 + 0.2, dim=-1).values
    d = torch.randn(R, 3, generator=gen)
    if degenerate and R >= R_DEG:
        dens[0] *= 0.02
        dens[5] *= 0.02
        dens[1, 0] = 1e4
        dens[2] = 0.0
        dens[3] = torch.linspace(0.0, 400.0, n) if n > 1 else torch.tensor([400.0])
        t[4, n // 2 + 1] = t[4, n // 2]
    return dict(rgb=rgb, density=dens, tdist=t, dirs=d, up_w=torch.randn(R, n, generator=gen), up_c=torch.randn(R, 3, generator=gen))


def mip_composite_oracle(inp, bg, dtype, which=("weights", "rgb")):
    c = lambda x: x.to(dtype)
    with torch.enable_grad():
        a, b = c(inp["rgb"]).clone().requires_grad_(True), c(inp["density"]).clone().requires_grad_(True)
        w = mip360.alpha_weights(b, c(inp["tdist"]), c(inp["dirs"]))
        col = (w[..., None] * a).sum(-2) + torch.clip(1 - w.sum(-1, keepdim=True), min=0) * bg
        loss = ((w * c(inp["up_w"])).sum() if "weights" in which else 0.0) + ((col * c(inp["up_c"])).sum() if "rgb" in which else 0.0)
        g_rgb, g_dens = torch.autograd.grad(loss, [a, b], allow_unused=True)
    zero = lambda g, like: torch.zeros_like(like) if g is None else g
    return dict(weights=_d(w), rgb=_d(col), g_rgb=zero(g_rgb, a), g_density=zero(g_dens, b))


def mip_composite_checks(got, ref64, ref32):
    checks = {}
    for k, const in (("weights", MIP_W), ("rgb", MIP_C)):
        if k in got:
            checks[k] = worst_entry(got[k], ref64[k], const, ref32[k])
    for k in ("g_rgb", "g_density"):
        if k in got:
            checks[k] = worst_entry(got[k], ref64[k], MIP_G * scale_of(ref64[k]), ref32[k])
    return checks


@functools.lru_cache(maxsize=None)
def mip_composite_case(n, bg, R=R_DEG, degenerate=True, which=("weights", "rgb")):
    inp = mip_composite_inputs(n, R, degenerate)
    return inp, mip_composite_oracle(inp, bg, torch.float64, which), mip_composite_oracle(inp, bg, torch.float32, which)
