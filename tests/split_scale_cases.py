"""Power-of-two rescalings of the NeO-360 decoder, the PixelNeRF decoder and the scene encoder's pillar stage: the low end of the
split-fp16 ("f16x3") arithmetic on the project's main path.  Plain CPU torch: tests/test_split_scale_cases_cpu.py checks the
conditions of every state on the very inputs that tests/test_gpu_split_scale_sweep.py hands to the kernels.  The table continues
dense_mlp_cases.py (vanilla and Mip-NeRF 360) and pillar_scale_cases.py (the high end of the pillar stage); scenes, point cases,
references and bounds are those of view_map_cases.py.

A ReLU network is unchanged when one layer (weight and bias) is multiplied by 2^-s and the layer that consumes its output by 2^s,
and in fp32 - where a power of two only moves the exponent of every product and partial sum - the output is the same bits in any
summation order (as long as nothing over- or underflows: checked on the CPU).  The split arithmetic is not invariant: hi = fp16(x)
keeps 11 bits only while x is an fp16 normal and lo = fp16(x - hi) underflows long before that, so an operand that is small
EVERYWHERE - a layer's weights, a feature map, a latent - loses accuracy.  Every state of the table can only trip the low end.

Point cases (both in V.CASES, so their references are cached): scene 7 (NV 3, planes 3 x 5, latent 5 x 7) at P = 63 = 9 rays x 7
samples with chunk 4, which does not divide R; scene 2 (NV 4, 12 x 16 / 24 x 32) at P = 203 = 7 x 29 = 6 x 32 + 11.  NeO-360 is
evaluated on the inside slot (fg_coarse_mlp) and the outside slot (bg_fine_mlp), PixelNeRF on V.PIX_SLOT.  Pillar cases: V.PILLAR 1
(NV 1, latent 5 x 7, grid 3,7,3, M = 63) and 3 (NV 5, grid 13,1,1, M = 65).

Kinds (DOWN x 2^-s, the compensation x 2^s):

  NeO-360 (both prefixes) and PixelNeRF (fine_mlp)
    T0  pts_linears.0 weight, bias            pts_linears.1.weight
    T1  pts_linears.1 weight, bias            pts_linears.2.weight
    T2  pts_linears.2 weight, bias            NeO-360: pts_linears.3.weight[:, :128] (the skip concatenation comes after layer 2);
                                              PixelNeRF: pts_linears.3.weight (no skip)
    V0  views_linear.0 weight, bias           views_linear.1.weight
    B   bottleneck_layer weight, bias         views_linear.0.weight[:, :128]
    F   NeO-360: the four scene maps          pts_linears.0.weight[:, 21 ch:] and pts_linears.3.weight[:, 128 + 21 ch:] (ch = 3
                                              inside, 4 outside)
        PixelNeRF: the latent                 pts_linears.0.weight[:, 63:]
  pillar stage
    P0  depth_fc.common_branch.0 weight, bias     depth_fc.common_branch.2.weight
    P1  depth_fc.common_branch.2 weight, bias     depth_fc.depth_encoder.weight
    A   pillar_aggregator_xz.0 weight, bias       pillar_aggregator_xz.2.weight
    L   the latent (a per-call operand)           depth_fc.common_branch.0.weight[:, :512]

Shifts: dense_mlp_cases.DOWN_SHIFTS; LAST_SHIFT gives, per kind, the largest shift whose compensated operand stays under 65504
(the CPU test recomputes it): 18 everywhere but pillar P0 (0.2899 x 2^18 = 76,000), P1 (0.3197 x 2^18 = 83,800) and L (0.3109 x
2^18 = 81,500), which end at 17.
"""
import contextlib
import functools

import torch
import torch.nn.functional as F

import dense_mlp_cases as D
import view_map_cases as V
from neo360_amd import synth

FP16_MAX = D.FP16_MAX
FP32_MIN_NORMAL = D.FP32_MIN_NORMAL
ORACLE_SHARE = D.ORACLE_SHARE
HALF = 0.5                   # an unflagged state may use this much of a bound (dense_mlp_sweep: the condition LOW rests on)

POINT_CASES = ((7, 63), (2, 203))                 # (scene index, P) of view_map_cases
PILLAR_CASES = (1, 3)                             # of V.PILLAR
# NeO-360 slots: name -> (slot, state prefix, input channels of the positional encoding)
NEO_SLOTS = {"inside": (V.FG_SLOT, V.FG_PREFIX, 3), "outside": (V.BG_SLOT, V.BG_PREFIX, 4)}
NEO_ALL_PREFIXES = (("fg_coarse_mlp.", 3), ("fg_fine_mlp.", 3), ("bg_coarse_mlp.", 4), ("bg_fine_mlp.", 4))
MAPS = ("plane_xz", "plane_xy", "plane_yz", "latent")

MLP_KINDS = ("T0", "T1", "T2", "V0", "B", "F")
KINDS = {"neo360": MLP_KINDS, "pixelnerf": MLP_KINDS, "pillar": ("P0", "P1", "A", "L")}
LAST_SHIFT = {("pillar", "P0"): 17, ("pillar", "P1"): 17, ("pillar", "L"): 17}      # every other kind: 18
MIDDLE_SHIFT = 10

# The low-end rule of the library (csrc/kernels.h; docs/split_scale_sweep.md derives every value from the measured curves): a
# linear layer with 0 < max |w| < LOW[family] trips the guard as a static operand; so does an uploaded feature map that a kernel
# splits raw with 0 < max |x| < LOW_MAP[family] (the three tri-planes are summed before the split: their common maximum counts);
# the pillar stage's latent is this call's input and trips per call.
LOW = {"neo360": 2.0 ** -11, "pixelnerf": 2.0 ** -9, "pillar": 2.0 ** -6}
LOW_MAP = {"neo360": 2.0 ** -8, "pixelnerf": 2.0 ** -8, "pillar": 2.0 ** -6}

# which maps a NeO-360 variant splits RAW, per slot (everything else is projected through the first-layer weights in fp32,
# k_tp_preproject): the default mode 3 projects the latent everywhere and the tri-planes outside the sphere only
NEO_SPLIT_VARIANTS = ("f16x3", "f16x3-pp1", "f16x3-pp2", "f16x3-noproj")
NEO_EXACT_VARIANTS = ("f32", "f32-pp1", "f32-noproj")
NEO_RAW_MAPS = {"f16x3": {"inside": ("planes",), "outside": ()},
                "f16x3-pp1": {"inside": ("planes",), "outside": ("planes",)},
                "f16x3-pp2": {"inside": (), "outside": ()},
                "f16x3-noproj": {"inside": ("planes", "latent"), "outside": ("planes", "latent")}}
# the layers of the decoder MLPs the split kernels never see as such: the pre-projected NeO-360 evaluators and both PixelNeRF
# evaluators fold bottleneck_layer into views_linear.0 in fp64 at pack time (k_fold_bottleneck), so its scale cancels exactly
NEO_FOLDED = {"f16x3": ("bottleneck_layer",), "f16x3-pp1": ("bottleneck_layer",), "f16x3-pp2": ("bottleneck_layer",), "f16x3-noproj": ()}
PIX_FOLDED = ("bottleneck_layer",)
PIX_VARIANTS = (True, False)                      # pre-projection of the latent on / off


def shifts(family, kind):
    last = LAST_SHIFT.get((family, kind), 18)
    return tuple(s for s in D.DOWN_SHIFTS if s < last) + (last,)


def states(family):
    """[(kind, shift)] of one family."""
    return [(k, s) for k in KINDS[family] for s in shifts(family, k)]


def _scale(sd, down, up, shift):
    """down: names multiplied by 2^-shift; up: (name, column slice) multiplied by 2^shift.  -> {label: scaled tensor}."""
    touched = {}
    for name in down:
        sd[name] = sd[name] * 2.0 ** -shift
        touched[name] = sd[name]
    for name, cols in up:
        w = sd[name].clone()
        w[:, cols] = w[:, cols] * 2.0 ** shift
        sd[name] = w
        touched["%s[:, %s:%s]" % (name, cols.start or "", cols.stop or "")] = w[:, cols]
    return touched


ALL = slice(None)


def _mlp_rescaling(prefix, kind, neo, ch=3):
    """-> (names scaled down, [(name, columns) scaled up]) of one decoder MLP for a weight kind."""
    wb = lambda layer: [prefix + layer + ".weight", prefix + layer + ".bias"]
    if kind == "T0":
        return wb("pts_linears.0"), [(prefix + "pts_linears.1.weight", ALL)]
    if kind == "T1":
        return wb("pts_linears.1"), [(prefix + "pts_linears.2.weight", ALL)]
    if kind == "T2":
        return wb("pts_linears.2"), [(prefix + "pts_linears.3.weight", slice(0, 128) if neo else ALL)]
    if kind == "V0":
        return wb("views_linear.0"), [(prefix + "views_linear.1.weight", ALL)]
    if kind == "B":
        return wb("bottleneck_layer"), [(prefix + "views_linear.0.weight", slice(0, 128))]
    if kind == "F":
        if neo:
            return [], [(prefix + "pts_linears.0.weight", slice(21 * ch, None)), (prefix + "pts_linears.3.weight", slice(128 + 21 * ch, None))]
        return [], [(prefix + "pts_linears.0.weight", slice(63, None))]
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def neo_base_state():
    return synth.nerf_tp_state(0)


@functools.lru_cache(maxsize=None)
def pix_base_state():
    return synth.pixelnerf_state(0)


def neo_state(kind, shift, s, prefixes=None):
    """-> (state dict, scene of case scene s, {label: scaled tensor}).  prefixes: [(prefix, input channels)] of the MLPs to rescale
    (default: the two evaluated slots; the frame tests rescale all four)."""
    sd = {k: v.clone() for k, v in neo_base_state().items()}
    sc = dict(V.scene_of(s))
    touched = {}
    for prefix, ch in (prefixes or [(p, c) for _, p, c in NEO_SLOTS.values()]):
        touched.update(_scale(sd, *_mlp_rescaling(prefix, kind, True, ch), shift))
    if kind == "F":
        for m in MAPS:
            sc[m] = sc[m] * 2.0 ** -shift
            touched[m] = sc[m]
    return sd, sc, touched


def pix_state(kind, shift, s):
    sd = {k: v.clone() for k, v in pix_base_state().items()}
    sc = dict(V.scene_of(s))
    touched = _scale(sd, *_mlp_rescaling(V.PIX_PREFIX, kind, False), shift)
    if kind == "F":
        sc["latent"] = sc["latent"] * 2.0 ** -shift
        touched["latent"] = sc["latent"]
    return sd, sc, touched


PILLAR_RESCALING = {"P0": ("depth_fc.common_branch.0", "depth_fc.common_branch.2.weight", ALL),
                    "P1": ("depth_fc.common_branch.2", "depth_fc.depth_encoder.weight", ALL),
                    "A": ("pillar_aggregator_xz.0", "pillar_aggregator_xz.2.weight", ALL),
                    "L": (None, "depth_fc.common_branch.0.weight", slice(0, 512))}
PILLAR_LAYERS = ("depth_fc.common_branch.0", "depth_fc.common_branch.2", "depth_fc.depth_encoder", "pillar_aggregator_xz.0",
                 "pillar_aggregator_xz.2", "pillar_aggregator_yz.0", "pillar_aggregator_yz.2", "pillar_aggregator_xy.0",
                 "pillar_aggregator_xy.2")          # the nine layers of neo_enc_upload


def pillar_state(kind, shift, i):
    """-> (params, latent, {label: scaled tensor}) of pillar case i."""
    c = V.pillar_case(i)
    p = {k: v.clone() for k, v in c["params"].items()}
    down, up, cols = PILLAR_RESCALING[kind]
    touched = _scale(p, [down + ".weight", down + ".bias"] if down else [], [(up, cols)], shift)
    lat = c["latent"]
    if kind == "L":
        lat = lat * 2.0 ** -shift
        touched["latent"] = lat
    return p, lat, touched


# ---- the rule the library applies, restated on the table ----------------------------------------------------------------------------
def _max(t):
    return float(t.abs().max())


def _inside(m, low):
    return 0.0 < m < low


def below_low(family, state, variant=None, slot=None):
    """True when the library's low-end rule flags `state` = what neo_state / pix_state / pillar_state return, on a split variant:
    neo360: variant of NEO_SPLIT_VARIANTS, slot 'inside' / 'outside'; pixelnerf: variant = pre-projection on (True) / off (False)."""
    sd, operand = state[0], state[1]
    if family == "pillar":
        return (any(_inside(_max(sd[l + ".weight"]), LOW[family]) for l in PILLAR_LAYERS) or _inside(_max(operand), LOW_MAP[family]))
    if family == "pixelnerf":
        prefix, folded = V.PIX_PREFIX, PIX_FOLDED
        raw = () if variant else ("latent",)
    else:
        prefix, folded = NEO_SLOTS[slot][1], NEO_FOLDED[variant]
        raw = NEO_RAW_MAPS[variant][slot]
    layers = [k for k in sd if k.startswith(prefix) and k.endswith(".weight") and k[len(prefix):-len(".weight")] not in folded]
    if any(_inside(_max(sd[k]), LOW[family]) for k in layers):
        return True
    if "planes" in raw and _inside(max(_max(operand[m]) for m in MAPS[:3]), LOW_MAP[family]):
        return True
    return "latent" in raw and _inside(_max(operand["latent"]), LOW_MAP[family])


def static_trip(family, kind):
    """What NeoRangeError.static_operand has to say for a flagged state: packed weights and uploaded maps are static operands, the
    pillar stage's latent is this call's input."""
    return not (family == "pillar" and kind == "L")


# ---- oracles --------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def linear_maxima():
    """Records, for every torch.nn.functional.linear call inside the block (the oracles' only matrix products), the largest |input| and
    |output|: yields the list of (max |x|, max |W x + b|)."""
    seen, plain = [], F.linear

    def spy(x, w, b=None):
        y = plain(x, w, b)
        seen.append((float(x.abs().max()), float(y.abs().max())))
        return y

    F.linear = spy
    try:
        yield seen
    finally:
        F.linear = plain


def evaluate(family, case, state, dtype=torch.float32):
    """The family's oracle on one case with `state`: neo360 -> (inside, outside), pixelnerf -> (out,), pillar -> (yz, xz, xy)."""
    if family == "neo360":
        return V.neo_eval(case[0], case[1], state[0], state[1], dtype)
    if family == "pixelnerf":
        return (V.pix_eval(case[0], case[1], state[0], state[1], dtype),)
    return V.pillar_eval(case, state[0], state[1], dtype)


def cases(family):
    return PILLAR_CASES if family == "pillar" else POINT_CASES


def make_state(family, kind, shift, case):
    if family == "neo360":
        return neo_state(kind, shift, case[0])
    if family == "pixelnerf":
        return pix_state(kind, shift, case[0])
    return pillar_state(kind, shift, case)


def base_state(family, case):
    if family == "neo360":
        return neo_base_state(), V.scene_of(case[0])
    if family == "pixelnerf":
        return pix_base_state(), V.scene_of(case[0])
    c = V.pillar_case(case)
    return c["params"], c["latent"]


@functools.lru_cache(maxsize=None)
def reference(family, case, dtype=torch.float64):
    """The base state's outputs, a tuple as `evaluate` returns it (the cached references of view_map_cases)."""
    if family == "neo360":
        return V.neo_reference(case[0], case[1], dtype)
    if family == "pixelnerf":
        return (V.pix_reference(case[0], case[1], dtype),)
    return V.pillar_reference(case, dtype)


def checks(family, case, got):
    """got: the tuple `evaluate` returns, from a kernel -> one {quantity: worst_entry} per output, under V.EVAL / V.PLAN."""
    ref64, ref32 = reference(family, case), reference(family, case, torch.float32)
    if family == "pillar":
        return [V.plan_checks(got, ref64, ref32)]
    return [V.eval_checks(g, a, b) for g, a, b in zip(got, ref64, ref32)]


def case_id(family, case):
    return "pillar%d" % case if family == "pillar" else "s%d-P%d" % case


def largest_operand(touched):
    """Largest |x| of the operand a state scaled DOWN (what the low-end rule looks at): the weight of the scaled layer, or the
    largest entry of the scaled maps."""
    return max(_max(t) for k, t in touched.items() if "[" not in k and not k.endswith(".bias"))
