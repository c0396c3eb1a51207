"""Case table, references and per-entry bounds for the dense point evaluators: the vanilla NeRF MLP (mlp_vanilla.hip,
mlp_vanilla_h.hip) and the Mip-NeRF 360 MLPs (mlp_mip.hip, mlp_mip_h.hip and the layer-by-layer schedule of mip_gemm_h.h /
mip_layered.h).  Plain CPU torch: tests/test_dense_mlp_cases_cpu.py checks the conditions of every case on the very inputs that
tests/test_gpu_dense_mlp_sweep.py hands to the kernels.

Shapes.  The Mip kernels work on tiles of 32 intervals (the layered schedule pads a batch to 2048), the vanilla kernels on tiles of
64 or 128 points: the point counts P = R x n sit on both sides of those edges, with odd n so that the g / n split of an interval
index and the (n + 1) row stride of tdist see more than 32, 64 and 128.

Bounds.  The constants of the single-shape tests (test_gpu_mip360.py, test_gpu_vanilla.py: 2e-5 on rgb and on density / sigma;
test_gpu_repeatable.py: 5e-6 between the split and the exact kernel), each times max(1, largest |fp64 value| of that output in the
case), entry by entry.

Power-of-two rescalings (SCALE_NETS, DOWN_SHIFTS, UP_SHIFT; compare pillar_scale_cases.py).  relu(2^-s (W1 h + b1)) = 2^-s
relu(W1 h + b1), so trunk layer 1 (weight and bias) x 2^-s with layer 2's weight x 2^s is the same network, and in fp32 - where a
power of two only moves the exponent of every product and partial sum - the same bits, in any summation order.  The split-fp16
arithmetic is not invariant: hi = fp16(x) keeps 11 bits only while x is an fp16 normal (|x| >= 6.1e-5) and lo = fp16(x - hi)
underflows long before that, so small weights lose accuracy (DOWN), and |x| >= 65504 does not fit at all (UP: the activations of
layer 1 leave the range while every weight stays inside both ends of it).
"""
import functools
import math

import torch

import alongray_cases as A
import cases
import oracle
from neo360_amd import synth
from oracle import mip360

RGB = 2e-5                 # test_gpu_mip360.py::test_mlp_stages_vs_oracle, test_gpu_vanilla.py::test_mlp_stage_vs_oracle
SIGMA = 2e-5
SPLIT_VS_EXACT = 5e-6      # test_gpu_repeatable.py: the split kernel against the exact kernel of the same case
ORACLE_SHARE = 1.0 / 3.0   # the fp32 oracle may use this much of a bound, no more

MIP_SHAPES = ((1, 1), (31, 1), (3, 11), (9, 7), (5, 13), (7, 29), (23, 89), (64, 32), (683, 3))      # P = 1 .. 2049
MIP_BITWISE_SHAPES = ((8191, 1), (2731, 3), (145, 113))       # 8191, 8193, 16385: layered against fused only
MIP_AUTO_SHAPES = ((8191, 1), (2731, 3))                      # either side of the automatic switch at 8192 intervals
MIP_GAIN = 0.5
# the 203-interval case again at weight_gain 1, where densities reach 0.8 and the outputs react 40 times more strongly to a wrong
# feature - and to the rounding of a correct fp32 evaluation: with the radii of the other cases the fp32 oracle itself uses 0.40 of
# the bounds (over the third a case may use), with cones four times as wide 0.25
MIP_STRONG = ((7, 29), 1.0, 4.0)                              # shape, weight_gain, radii x
MIP_DEG = (9, 7)
VANILLA_SHAPES = ((1, 1), (9, 7), (8, 8), (5, 13), (127, 1), (2, 64), (3, 43), (7, 29), (257, 1))    # P = 1 .. 257
VANILLA_DEG = (9, 7)
VANILLA_LEVELS = (("coarse_mlp.", 0), ("fine_mlp.", 1))
NEAR, FAR = 0.2, 3.0
STRADDLE_ROW = 8           # the row of the 9 x 7 Mip case built to cross |x| = 1 (rows 6 and 7 are the ordinary ones)

FP16_MAX = 65504.0
FP32_MIN_NORMAL = 2.0 ** -126


def shape_id(shape):
    return "%dx%d" % shape


# ---- vanilla NeRF --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vanilla_inputs(R, N):
    """rays_o (R,3), dirs (R,3), t (R,N) ascending in [0.2, 3.0].  The 9 x 7 case: row 0 has two equal t, row 1 has dirs = 0 (every
    point of the ray is its origin), row 2 has |dirs| = 1.7."""
    rays = cases.strided_rays(R)
    o, d = rays["rays_o"].clone(), rays["viewdirs"].clone()
    t = torch.sort(synth.uniform(83, "dense_v_t_%d_%d" % (R, N), (R, N), NEAR, FAR), dim=-1).values
    if (R, N) == VANILLA_DEG:
        t[0, 4] = t[0, 3]
        d[1] = 0.0
        d[2] = d[2] * 1.7
    return dict(rays_o=o, dirs=d, t=t.contiguous())


def vanilla_oracle(params, prefix, inp, dtype):
    """(R,N,4) = (rgb, sigma) after the activations, as NeRF.eval_mlp returns them."""
    c = lambda x: x.to(dtype)
    p = {k: c(v) for k, v in params.items() if k.startswith(prefix)}
    pts = oracle.sampling.points_on_rays(c(inp["t"]), c(inp["rays_o"]), c(inp["dirs"]))
    raw_rgb, raw_sigma = oracle.mlp.vanilla_mlp(p, prefix, oracle.encoding.pos_enc(pts, 0, 10), oracle.encoding.pos_enc(c(inp["dirs"]), 0, 4))
    return torch.cat([oracle.mlp.colour_activation(raw_rgb), oracle.mlp.density_activation(raw_sigma)], dim=-1)


@functools.lru_cache(maxsize=None)
def vanilla_reference(R, N, prefix, dtype=torch.float64):
    return vanilla_oracle(synth.vanilla_state(0), prefix, vanilla_inputs(R, N), dtype)


# ---- Mip-NeRF 360 --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mip_inputs(R, n, radii_gain=1.0):
    """The batch (rays_o, rays_d, viewdirs, radii) and tdist (R, n+1) ascending in [0.2, 3.0].  The 9 x 7 case: row 0 a zero-width
    interval, row 1 radius 0, row 2 starts at -d and runs through the world origin (t 0.7 .. 1.3), row 3 reaches t = 1e6 (the row of
    test_gpu_repeatable.py), rows 4 / 5 have rays_d x 5 / x 0.01, rows 6 and 7 are ordinary, row 8 spans 0.3 either side of the
    point where the ray leaves the unit ball (the branch of the contraction)."""
    rays = {k: v.clone() for k, v in cases.mip_rays(R).items()}
    s = torch.sort(synth.uniform(83, "dense_m_s_%d_%d" % (R, n), (R, n + 1), 0.0, 1.0), dim=-1).values
    tdist = 1 / (s * (1 / FAR) + (1 - s) * (1 / NEAR))
    rays["radii"] = rays["radii"] * radii_gain
    if (R, n) == MIP_DEG:
        tdist[0, 4] = tdist[0, 3]
        rays["radii"][1] = 0.0
        rays["rays_o"][2] = -rays["rays_d"][2]
        tdist[2] = torch.linspace(0.7, 1.3, n + 1)
        e = torch.linspace(0.0, 1.0, n + 1)
        tdist[3] = 1.0 / (e / 1e6 + (1.0 - e) / 0.2)
        rays["rays_d"][4] = rays["rays_d"][4] * 5.0
        rays["rays_d"][5] = rays["rays_d"][5] * 0.01
        o, d = rays["rays_o"][STRADDLE_ROW].double(), rays["rays_d"][STRADDLE_ROW].double()
        a, b, c = float(d @ d), float(2 * (o @ d)), float(o @ o) - 1.0          # |o + t d| = 1
        t_exit = (-b + (b * b - 4 * a * c) ** 0.5) / (2 * a)
        tdist[STRADDLE_ROW] = torch.linspace(t_exit - 0.3, t_exit + 0.3, n + 1)
    return rays, tdist.contiguous()


def mip_means(R, n, dtype=torch.float64):
    rays, tdist = mip_inputs(R, n)
    c = lambda x: x.to(dtype)
    return mip360.conical_frustum_gaussians(c(tdist), c(rays["rays_o"]), c(rays["rays_d"]), c(rays["radii"]))[0]


def mip_oracle(params, slot, rays, tdist, dtype):
    """(R,n,4) = (rgb, density), as MipNeRF360.eval_mlp returns them (a proposal MLP has no colour: zeros)."""
    c = lambda x: x.to(dtype)
    prefix = "mlps.%d." % slot
    p = {k: c(v) for k, v in params.items() if k.startswith(prefix)}
    means, covs = mip360.conical_frustum_gaussians(c(tdist), c(rays["rays_o"]), c(rays["rays_d"]), c(rays["radii"]))
    nerf = slot == 2
    dens, col = mip360.mlp(p, prefix, c(mip360.icosahedron_basis()), means, covs, c(rays["viewdirs"]), 8 if nerf else 4, nerf)
    return torch.cat([col, dens[..., None]], dim=-1)


@functools.lru_cache(maxsize=None)
def mip_state(gain=MIP_GAIN):
    return synth.mip360_state(0, weight_gain=gain)


@functools.lru_cache(maxsize=None)
def mip_reference(R, n, slot, gain=MIP_GAIN, dtype=torch.float64, radii_gain=1.0):
    rays, tdist = mip_inputs(R, n, radii_gain)
    return mip_oracle(mip_state(gain), slot, rays, tdist, dtype)


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
def eval_checks(got, ref64, ref32=None):
    """(.., 4) = (rgb, density or sigma) -> {quantity: worst_entry}, each constant x max(1, largest |fp64 value| of that output)."""
    got = torch.as_tensor(got).detach().cpu()
    pick = lambda x, sl: None if x is None else x[..., sl]
    return dict(rgb=A.worst_entry(got[..., :3], ref64[..., :3], RGB * A.scale_of(ref64[..., :3]), pick(ref32, slice(0, 3))),
                sigma=A.worst_entry(got[..., 3], ref64[..., 3], SIGMA * A.scale_of(ref64[..., 3]), pick(ref32, 3)))


def split_vs_exact_checks(split, exact, ref64):
    """The split kernel's output against the exact kernel's on the same case: 5e-6 x the same scales."""
    split, exact = torch.as_tensor(split).detach().cpu(), torch.as_tensor(exact).detach().cpu().double()
    return dict(rgb_vs_f32=A.worst_entry(split[..., :3], exact[..., :3], SPLIT_VS_EXACT * A.scale_of(ref64[..., :3])),
                sigma_vs_f32=A.worst_entry(split[..., 3], exact[..., 3], SPLIT_VS_EXACT * A.scale_of(ref64[..., 3])))


# ---- power-of-two rescalings ---------------------------------------------------------------------------------------------------------
# net -> (state prefix, name of the trunk list, the case the scaled states are evaluated on)
SCALE_NETS = {"vanilla": ("coarse_mlp.", "pts_linears"), "mip_prop": ("mlps.0.", "pts_linear"), "mip_nerf": ("mlps.2.", "pts_linear")}
DOWN_SHIFTS = (4, 6, 8, 10, 12, 14, 18)
# UP: the largest shift that keeps every scaled weight below 65504 while the activations of layer 1 reach it (checked on the CPU).
# mlps.2 at 2^20: max |w1| 4.0e4, max h1 9.1e5; mlps.0 needs 2^19 (2^20 takes its w1 to 8.0e4); coarse_mlp 2^19: see the CPU test.
UP_SHIFT = {"vanilla": 19, "mip_prop": 19, "mip_nerf": 20}
# The static low-end check of the split arithmetic (csrc/kernels.h SPLIT_WEIGHT_LOW): a linear layer with 0 < max |w| < LOW trips
# the range guard as a static operand.  docs/dense_mlp_sweep.md derives the value from the measured curve: the DOWN states that
# used more than half a bound have max |w1| <= 2^-15.2, those with max |w1| >= 2^-13.7 used at most 0.36 of it.
LOW = 2.0 ** -13


def base_state(net):
    return synth.vanilla_state(0) if net == "vanilla" else mip_state(MIP_GAIN)


# the layers behind trunk layer 1 that an UP state spreads its compensation over: all in front of the skip concatenation (layer
# 5 reads [h4 | encoding], so h4 has to be back at its own scale); the proposal MLP has four trunk layers and ends in the density head
UP_COMPENSATE = {"vanilla": ("pts_linears.2", "pts_linears.3", "pts_linears.4"), "mip_prop": ("pts_linear.2", "pts_linear.3", "density_layer"),
                 "mip_nerf": ("pts_linear.2", "pts_linear.3", "pts_linear.4")}


def scaled_state(net, shift, up=False):
    """-> (state dict, {name: scaled tensor}).
    DOWN: trunk layer 1 (weight, bias) x 2^-shift, layer 2's weight x 2^shift.
    UP: layer 1 (weight, bias) x 2^shift; the inverse is SPREAD over the layers of UP_COMPENSATE, each weight by the largest power
    of two that keeps its max |w| at or above LOW, each bias by what is left of the shift behind its layer.  (Layer 2 alone x
    2^-shift - the mirror image of DOWN - would put that layer under LOW: the state would trip the static low-end check and say
    nothing about the guard on the activations.)"""
    prefix, trunk = SCALE_NETS[net]
    sd = {k: v.clone() for k, v in base_state(net).items()}
    w1, b1 = "%s%s.1.weight" % (prefix, trunk), "%s%s.1.bias" % (prefix, trunk)
    if not up:
        names = (w1, b1, "%s%s.2.weight" % (prefix, trunk))
        for name, f in zip(names, (2.0 ** -shift, 2.0 ** -shift, 2.0 ** shift)):
            sd[name] = sd[name] * f
        return sd, {k: sd[k] for k in names}
    scaled = [w1, b1]
    sd[w1], sd[b1] = sd[w1] * 2.0 ** shift, sd[b1] * 2.0 ** shift
    left = shift
    for layer in UP_COMPENSATE[net]:
        w, b = prefix + layer + ".weight", prefix + layer + ".bias"
        k = min(left, int(math.floor(math.log2(float(sd[w].abs().max()) / LOW))))
        left -= k
        sd[w], sd[b] = sd[w] * 2.0 ** -k, sd[b] * 2.0 ** left
        scaled += [w, b]
    assert left == 0, (net, shift, left)
    return sd, {k: sd[k] for k in scaled}


def scale_states():
    """[(net, 'down' | 'up', shift)] of the whole table."""
    return [(net, "down", s) for net in SCALE_NETS for s in DOWN_SHIFTS] + [(net, "up", UP_SHIFT[net]) for net in SCALE_NETS]


def scale_oracle(net, state, dtype):
    """The 9 x 7 case of the net's family through the oracle with `state`."""
    if net == "vanilla":
        return vanilla_oracle(state, SCALE_NETS[net][0], vanilla_inputs(*VANILLA_DEG), dtype)
    rays, tdist = mip_inputs(*MIP_DEG)
    return mip_oracle(state, int(SCALE_NETS[net][0][5]), rays, tdist, dtype)


@functools.lru_cache(maxsize=None)
def scale_reference(net, dtype=torch.float64):
    return scale_oracle(net, base_state(net), dtype)


def layer1_activations(net, state, behind=False):
    """fp32 activations behind trunk layer 1 of `state` on the net's 9 x 7 case (what the split kernel has to hold in fp16);
    behind=True: the largest activation behind each later trunk layer in front of the skip concatenation instead."""
    prefix, trunk = SCALE_NETS[net]
    if net == "vanilla":
        inp = vanilla_inputs(*VANILLA_DEG)
        x0 = oracle.encoding.pos_enc(oracle.sampling.points_on_rays(inp["t"], inp["rays_o"], inp["dirs"]), 0, 10)
    else:
        rays, tdist = mip_inputs(*MIP_DEG)
        means, covs = mip360.conical_frustum_gaussians(tdist, rays["rays_o"], rays["rays_d"], rays["radii"])
        lm, lv = mip360.lift_and_diagonalize(*mip360.contract(means, covs), mip360.icosahedron_basis())
        x0 = mip360.integrated_pos_enc(lm, lv, 0, 12)
    h = x0
    for i in range(2):
        h = torch.relu(torch.nn.functional.linear(h, state["%s%s.%d.weight" % (prefix, trunk, i)], state["%s%s.%d.bias" % (prefix, trunk, i)]))
    if not behind:
        return h
    later = []
    for i in range(2, 5 if net != "mip_prop" else 4):
        h = torch.relu(torch.nn.functional.linear(h, state["%s%s.%d.weight" % (prefix, trunk, i)], state["%s%s.%d.bias" % (prefix, trunk, i)]))
        later.append(float(h.abs().max()))
    return later


def layer_weight_maxima(net, state):
    """{layer name: max |w|} over the linear layers of the net's MLP (the operands the split arithmetic packs)."""
    prefix = SCALE_NETS[net][0]
    return {k: float(v.abs().max()) for k, v in state.items() if k.startswith(prefix) and k.endswith(".weight")}


def below_low(net, state, low=None):
    """True when some layer of the MLP has 0 < max |w| < LOW: the state the static low-end check flags."""
    low = LOW if low is None else low
    return any(0.0 < m < low for m in layer_weight_maxima(net, state).values())
