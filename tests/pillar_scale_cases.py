"""Power-of-two rescalings of the pillar stage's operands (importable on the CPU; used by test_pillar_scale_cases_cpu.py and
test_gpu_encoder_f32.py).

Multiplying an fp32 number by a power of two is exact as long as neither the product over- nor underflows, and ReLU commutes
with a positive scale.  So an operand of a linear layer can be pushed far beyond the fp16 range (|x| >= 65504: the range guard
of the split arithmetic trips) while the layer that consumes it is compensated by the inverse power: every product, every
partial sum and therefore every fp32 RESULT stays bitwise what it was, in any summation order.  An exact-fp32 evaluator must
return `torch.equal` floor-plans for the scaled and the unscaled operands; the split-fp16 evaluator cannot run the scaled ones.

  case L (the latent, a per-call operand):   latent x 2^17,  depth_fc.common_branch.0.weight[:, :512] x 2^-17
  case W (a packed weight, a static operand): depth_fc.common_branch.2.weight x 2^18,
                                              depth_fc.common_branch.0.weight and .bias x 2^-18
                                              (h1 = relu(W0 x + b0) shrinks by 2^-18, W1 h1 is unchanged)

Case W was first written with 2^17 like case L.  The CPU test showed that this does not leave the fp16 range: the largest
|depth_fc.common_branch.2.weight| of synth.pillar_state(0) is 0.2963 (kaiming normal, std 1/16, 262,144 draws), 2^17 takes it
to 38,839 < 65,504, and the split arithmetic would simply run.  One more doubling gives 77,678: beyond fp16, with every
assertion of the case kept as it was (bitwise invariance of the fp32 oracle, largest operand >= 65504, nothing subnormal).
"""
import torch

SHIFT = 17                       # case L, and the decoder compensation that goes with it
UP = float(2 ** SHIFT)
DOWN = float(2.0 ** -SHIFT)
SHIFT_W = 18                     # case W: see above
UP_W = float(2 ** SHIFT_W)
DOWN_W = float(2.0 ** -SHIFT_W)
FP16_MAX = 65504.0
FP32_MIN_NORMAL = 2.0 ** -126

W0 = "depth_fc.common_branch.0.weight"
B0 = "depth_fc.common_branch.0.bias"
W1 = "depth_fc.common_branch.2.weight"


def case_l(params, latent):
    """-> (scaled params, scaled latent, the operands that were scaled: name -> tensor)."""
    p = {k: v.clone() for k, v in params.items()}
    p[W0][:, :512] *= DOWN
    lat = latent * UP
    return p, lat, {"latent": lat, W0 + "[:, :512]": p[W0][:, :512]}


def case_w(params, latent):
    p = {k: v.clone() for k, v in params.items()}
    p[W1] *= UP_W
    p[W0] *= DOWN_W
    p[B0] *= DOWN_W
    return p, latent.clone(), {W1: p[W1], W0: p[W0], B0: p[B0]}


CASES = {"L": case_l, "W": case_w}


def largest(scaled):
    return max(float(t.abs().max()) for t in scaled.values())


def smallest_nonzero(scaled):
    return min(float(t[t != 0].abs().min()) for t in scaled.values() if bool((t != 0).any()))


def decoder_compensated(state, input_chs=(("fg_coarse_mlp.", 3), ("fg_fine_mlp.", 3), ("bg_coarse_mlp.", 4), ("bg_fine_mlp.", 4))):
    """NeRF_TP decoder weights for a latent scaled by 2^17: the local-latent columns of the four NeRFPPMLPs x 2^-17.  The input of
    pts_linears.0 is [pos_enc (21 input_ch) | local latent 512 | tri-plane 128]; pts_linears.3 takes [h (128) | that input]."""
    sd = {k: v.clone() for k, v in state.items()}
    for prefix, ch in input_chs:
        pe = 21 * ch
        sd[prefix + "pts_linears.0.weight"][:, pe:pe + 512] *= DOWN
        sd[prefix + "pts_linears.3.weight"][:, 128 + pe:128 + pe + 512] *= DOWN
    return sd
